# -*- coding: utf-8 -*-
"""K25 (xc_contour_map) without a GPU: the restatement of its rule (cmap_ref.py) against values worked out by hand; deliberately
wrong variants of it must disagree with it on the inputs the gpu tests run, class by class, so that none of those can pass
vacuously; and the host layer above the library -- the binding's batching and the facade's validation -- over the stand-in library."""
import numpy as np
import pytest

import cmap_ref as R
import standin_lib
from standin_lib import RES, _Lib

import xcontour_amd as xa
from xcontour_amd import _native as nat

NAN, INF = np.nan, np.inf


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return bool(((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def _one(q, xp, fp, out_dtype=np.float64):
    return R.contour_map(np.asarray(q, dtype=np.float64).reshape(1, 1, -1), xp, [fp], out_dtype)[0].ravel()


# ---------------------------------------------------------------------------------------------------- the rule, by hand
def test_restatement_by_hand():
    xp, fp = [0.0, 1.0, 3.0], [10.0, 20.0, 0.0]
    # exact hits return F(j) itself, both ends included; inside: slope * (x - X[j]) + F[j]
    assert _same(_one([0.0, 1.0, 3.0], xp, fp), [10.0, 20.0, 0.0])
    assert _same(_one([0.25, 2.0], xp, fp), [12.5, 10.0])
    # both clamps, the infinities with them; NaN stays NaN; -0.0 is the level 0.0
    assert _same(_one([-5.0, 7.0, -INF, INF, NAN, -0.0], xp, fp), [10.0, 0.0, 10.0, 0.0, NAN, 10.0])
    # decreasing levels: both arrays reversed (core.py:1428-1430)
    assert _same(_one([0.25, 2.0, -1.0, 4.0, 3.0], xp[::-1], fp[::-1]), [12.5, 10.0, 10.0, 0.0, 0.0])
    assert _same(_one([0.25], xp[::-1], fp), [0.0 + (20.0 - 0.0) * 0.25])         # ... the vector is reversed WITH them
    # NaN in fp at j + 1: both formulas give NaN and the ends differ -> NaN; but the exact hit on j returns F(j)
    assert _same(_one([0.5, 0.0], xp, [10.0, NAN, 0.0]), [NAN, 10.0])
    # NaN in fp at j: NaN, and the exact hit returns that NaN; the clamp beyond returns the end value
    assert _same(_one([1.5, 1.0, 3.0, 9.0], xp, [10.0, NAN, 0.0]), [NAN, NAN, 0.0, 0.0])
    # an infinite end: slope inf, first formula inf * dx + F; at x next to the other end still inf
    assert _same(_one([0.5], xp, [10.0, INF, 0.0]), [INF])
    assert _same(_one([2.0], xp, [10.0, INF, 0.0]), [INF])                         # slope -inf: -inf * 1 + inf = NaN, then -inf * -1 + 0
    assert _same(_one([2.0], xp, [10.0, -INF, 5.0]), [-INF])                       # slope +inf: inf * 1 - inf = NaN, then inf * -1 + 5
    # equal infinite ends: slope NaN, both formulas NaN, F(j + 1) == F(j): numpy's last fall-back returns F(j)
    assert _same(_one([0.5], xp, [INF, INF, 0.0]), [INF])
    # equal END LEVELS (not xp[0] < xp[-1]): the reversed direction
    assert _same(_one([0.5, 2.0], [1.0, 1.0], [3.0, 4.0]), [4.0, 3.0])
    # a slab whose first or last level is NaN: NaN everywhere
    assert _same(_one([0.5, NAN, 9.0], [NAN, 1.0, 2.0], fp), [NAN, NAN, NAN])
    assert _same(_one([0.5], [0.0, 1.0, NAN], fp), [NAN])
    # float32 output: the float64 result rounded once
    v = _one([1.0 / 3.0], xp, [0.0, 1.0, 0.0], np.float32)
    assert v.dtype == np.float32 and v[0] == np.float32(1.0 / 3.0)
    # a float32 tracer is promoted, never the levels demoted
    q32 = np.array([[[0.1]]], dtype=np.float32)
    assert _same(R.contour_map(q32, xp, [fp])[0], [10.0 + 10.0 * float(np.float32(0.1))])


def test_restatement_per_slab_and_shared():
    xp = np.array([[0.0, 1.0, 2.0], [2.0, 1.0, 0.0]])
    f0, f1 = np.array([1.0, 2.0, 4.0]), np.array([[0.0, 0.0, 1.0], [5.0, 6.0, 7.0]])
    q = np.array([[[0.5, 1.5]], [[0.5, 1.5]]])
    a, b = R.contour_map(q, xp, [f0, f1])
    assert _same(a, [1.5, 3.0, 3.0, 1.5]) and _same(b, [0.0, 0.5, 6.5, 5.5])


def test_refusals_restated():
    ok = np.linspace(0, 1, 5)
    assert R.refusal(1, 5, 1, ok) == R.XC_OK
    assert R.refusal(1, 1, 1) == R.refusal(1, 5, 0) == R.refusal(1, 5, 9) == R.refusal(0, 5, 1) == R.XC_EBADARG
    assert R.refusal(1, 4096, 1) == R.XC_OK and R.refusal(1, 4097, 1) == R.XC_EBADARG
    assert R.refusal(1, 910, 8) == R.XC_OK and R.refusal(1, 911, 8) == R.XC_EBADARG
    assert R.refusal(1, 3000, 1) == R.refusal(1, 201, 8) == R.XC_OK
    assert R.refusal(65535, 2, 1) == R.XC_OK and R.refusal(65536, 2, 1) == R.XC_EBADARG
    assert R.refusal(1, 5, 1, ok, q_dtype=np.int32) == R.XC_EBADARG
    assert R.refusal(1, 5, 1, [0, 1, 1, 2, 3]) == R.XC_EEDGES
    assert R.refusal(1, 5, 1, [0, 2, 1, 3, 4]) == R.XC_EBADARG and R.refusal(1, 5, 1, [0, 1, INF, 3, 4]) == R.XC_EBADARG
    assert R.refusal(1, 5, 1, [0, 2, 1, 3, 4], host=False) == R.XC_OK            # the device form cannot read them
    assert R.refusal(2, 3, 1, [[NAN, 1, 1], [3, 2, 1]]) == R.XC_OK               # an all-NaN tracer's levels are let through


# ---------------------------------------------------------------------------------------------------- no case passes vacuously
def _gpu_inputs():
    """(class, q, xp, fps) over the kinds of levels, vectors and tracers the gpu tests run, on their (5, 257) plane"""
    for kind in ('linear', 'geometric', 'gap'):
        for dec in (False, True):
            for N in (2, 3, 64, 65, 201):
                xp = R.levels(kind, N, dec)
                fps = [R.values(k, N, i) for i, k in enumerate(('finite', 'nan', 'inf', 'flat_inf'))]
                for base in ('smooth', 'noise'):
                    yield ('decreasing' if dec else 'increasing'), R.stack(xp, 1, 5, 257, np.float64, base, N), xp, fps


def test_steps_are_numpy_and_wrong_variants_disagree():
    caught = {'clamp': 0, 'reversal': 0, 'hit': 0, 'f32': 0}
    for cls, q, xp, fps in _gpu_inputs():
        ref = R.contour_map(q, xp, fps)
        for a, b in zip(R.variant(q, xp, fps), ref):
            assert _same(a, b)                                  # the steps, unflagged, ARE np.interp: the variants below differ by their flag alone
        fin = fps[:1]
        caught['clamp'] += not _same(R.variant(q, xp, fin, clamp=False)[0], ref[0])
        caught['hit'] += not _same(R.variant(q, xp, fin, hit_right=True)[0], ref[0])
        caught['f32'] += not _same(R.variant(q, xp, fin, ft=np.float32)[0], ref[0])
        if cls == 'decreasing':
            caught['reversal'] += not _same(R.variant(q, xp, fin, reversal=False)[0], ref[0])
    n = len(list(_gpu_inputs()))
    # every input reaches past both ends, holds every level exactly, and is float64; half of them run on decreasing levels
    assert caught == {'clamp': n, 'reversal': n // 2, 'hit': n, 'f32': n}, caught


def test_gpu_inputs_hold_what_they_promise():
    xp = R.levels('gap', 65)
    q = R.tracer(xp, 5 * 257, np.float64)
    for v in np.concatenate((xp, np.nextafter(xp, -INF), np.nextafter(xp, INF))):
        assert (q == v).any()
    assert np.isnan(q).any() and (q == INF).any() and (q == -INF).any() and (q < xp[0]).any() and (q > xp[-1]).any()
    assert np.signbit(q[q == 0.0]).any()
    # the uniform guess of the gap levels misses by more than N / 2 for every node in the upper half of [0, 1]
    guess = np.floor((0.75 - xp[0]) * (len(xp) - 1) / (xp[-1] - xp[0]))
    assert np.searchsorted(xp, 0.75, side='right') - 1 - guess > len(xp) / 2
    # float32-representable levels stay strictly monotonic, and a float32 tracer hits them exactly
    x32 = R.levels('geometric', 201, f32=True)
    q32 = R.tracer(x32, 2000, np.float32)
    assert np.isin(x32, q32.astype(np.float64)).all()
    # smooth: neighbours share brackets; noise: they do not
    xs = R.levels('linear', 201)
    js = lambda q: np.searchsorted(xs, q[1000:].astype(np.float64))
    assert (np.diff(js(R.tracer(xs, 33 * 1025, np.float64, 'smooth'))) == 0).mean() > 0.9
    assert (np.diff(js(R.tracer(xs, 33 * 1025, np.float64, 'noise'))) == 0).mean() < 0.1


# ---------------------------------------------------------------------------------------------------- the host layer, stand-in library
S, NY, NX, N = 5, 6, 8, 4


@pytest.fixture
def ctx(monkeypatch):
    monkeypatch.setitem(standin_lib._NSLAB_ARG, 'xc_contour_map', 3)
    monkeypatch.setitem(standin_lib._NSLAB_ARG, 'xc_contour_map_dev', 3)
    c = nat.Context.__new__(nat.Context)
    c.lib, c.handle, c.device = _Lib(), None, 0
    c._buffers, c._resident, c._staged, c._ev_pool = [], {}, [], []
    c.max_batch_bytes = 8 << 30
    return c


def _calls(ctx):
    out, ctx.lib.calls = ctx.lib.calls, []
    return out


def test_binding_batches_with_the_outputs_in_the_budget(ctx):
    q = np.random.default_rng(7).standard_normal((S, NY, NX))
    lev, f = np.linspace(-1, 1, N), np.arange(N, dtype=float)
    slab = NY * NX * 8
    out = ctx.contour_map(q, lev, [f])
    assert _calls(ctx) == [('xc_contour_map', S)]
    assert type(out) is list and len(out) == 1 and out[0].shape == (S, NY, NX) and out[0].dtype == np.float64
    ctx.max_batch_bytes = 2 * slab * 2 + 8                           # tracer + one float64 plane per slab: two slabs fit
    out = ctx.contour_map(q, lev, [f])
    assert _calls(ctx) == [('xc_contour_map', 2), ('xc_contour_map', 2), ('xc_contour_map', 1)]
    assert type(out) is list and out[0].shape == (S, NY, NX)
    out = ctx.contour_map(q, np.tile(lev, (S, 1)), [f, np.tile(f, (S, 1)), f])        # three planes: 4 x 8 bytes per cell, one slab fits
    assert _calls(ctx) == [('xc_contour_map', 1)] * S
    assert len(out) == 3 and all(o.shape == (S, NY, NX) for o in out)
    ctx.max_batch_bytes = 2 * (slab + 3 * NY * NX * 4) + 8           # float32 planes count 4 bytes
    out = ctx.contour_map(q, lev, [f, f, f], out_dtype=np.float32)
    assert _calls(ctx) == [('xc_contour_map', 2), ('xc_contour_map', 2), ('xc_contour_map', 1)]
    assert all(o.dtype == np.float32 and o.shape == (S, NY, NX) for o in out)
    # the per-slab arrays of a batch are that batch's rows; shared ones go whole
    ctx.lib.args = []
    ctx.contour_map(q, np.tile(lev, (S, 1)) + np.arange(S)[:, None], [f])
    a = [x for n, x in ctx.lib.args if n == 'xc_contour_map']
    assert [x[3] for x in a] == [2, 2, 1] and [x[7:10] for x in a] == [(N, 1, 1)] * 3


def test_binding_resident_tracer_goes_to_the_dev_entry(ctx):
    q = np.random.default_rng(7).standard_normal((S, NY, NX))
    ctx._resident[q.ctypes.data] = q
    ctx.lib.resident_base = q.ctypes.data
    ctx.max_batch_bytes = 2 * NY * NX * 16 + 8
    out = ctx.contour_map(q, np.linspace(-1, 1, N), [np.arange(N, dtype=float)])
    assert _calls(ctx) == [('xc_contour_map_dev', 2), ('xc_contour_map_dev', 2), ('xc_contour_map_dev', 1)]
    a = [x for n, x in ctx.lib.args if n == 'xc_contour_map_dev']
    assert [x[1] for x in a] == [RES, RES + 2 * NY * NX * 8, RES + 4 * NY * NX * 8]         # the mirror, read in place: no upload of the tracer
    assert out[0].shape == (S, NY, NX) and ctx._buffers == []
    # the device form trusts its caller: the binding checks the levels as the host form does, with its codes
    with pytest.raises(nat.XContourHipError) as e:
        ctx.contour_map(q, [0.0, 1.0, 1.0, 2.0], [np.arange(N, dtype=float)])
    assert e.value.code == nat.XC_EEDGES and str(e.value) == 'non monotonic bins'
    with pytest.raises(nat.XContourHipError) as e:
        ctx.contour_map(q, [0.0, 2.0, 1.0, 3.0], [np.arange(N, dtype=float)])
    assert e.value.code == nat.XC_EBADARG


def test_binding_refuses_what_the_library_would(ctx):
    q = np.zeros((S, NY, NX))
    lev, f = np.linspace(-1, 1, N), np.arange(N, dtype=float)
    for bad in (lambda: ctx.contour_map(q[0], lev, [f]), lambda: ctx.contour_map(q, lev[:1], [f[:1]]),
                lambda: ctx.contour_map(q, np.tile(lev, (S + 1, 1)), [f]), lambda: ctx.contour_map(q, lev, []),
                lambda: ctx.contour_map(q, lev, [f] * 9), lambda: ctx.contour_map(q, lev, [f[:-1]]),
                lambda: ctx.contour_map(q, lev, [np.tile(f, (S - 1, 1))]), lambda: ctx.contour_map(q, lev, [f], out_dtype=np.int32),
                lambda: ctx.contour_map(q, np.linspace(0, 1, 4097), [np.zeros(4097)])):
        with pytest.raises(nat.XContourHipError) as e:
            bad()
        assert e.value.code == nat.XC_EBADARG
    assert _calls(ctx) == []
    ctx.contour_map(q, np.linspace(0, 1, 4096), [np.zeros(4096)])
    assert _calls(ctx) == [('xc_contour_map', S)]


# ---------------------------------------------------------------------------------------------------- facade validation
@pytest.fixture
def cm(ctx, monkeypatch):
    monkeypatch.setattr(nat, 'default_context', lambda device=0: ctx)
    monkeypatch.setattr(xa, 'default_context', lambda device=0: ctx)
    lat, lon, t = np.linspace(-60, 60, NY), np.linspace(0, 315, NX), np.arange(3.0)
    q = np.random.default_rng(3).standard_normal((3, NY, NX))
    tr = xa.DataArray(q, ('time', 'latitude', 'longitude'), {'time': t, 'latitude': lat, 'longitude': lon}, 'pv')
    return xa.Contour2D(tr, np.ones((NY, NX)), dims={'X': 'longitude', 'Y': 'latitude'}, dimEq={'Y': 'latitude'}, increase=True, lt=True)


def _vec(shape_dims, name, n=N, **lead):
    dims = tuple(lead) + ('contour',)
    shape = tuple(len(v) for v in lead.values()) + (n,)
    c = dict(lead)
    c['contour'] = np.arange(n, dtype=float)
    return xa.DataArray(np.arange(int(np.prod(shape)), dtype=float).reshape(shape), dims, c, name)


def test_facade_shapes_names_and_validation(cm, ctx):
    t = np.arange(3.0)
    ctr = _vec(None, 'pv', time=t)
    one = cm.map_to_plane(ctr, _vec(None, 'latEq', time=t))
    assert _calls(ctx) == [('xc_contour_map', 3)]
    assert one.dims == ('time', 'latitude', 'longitude') and one.shape == (3, NY, NX) and one.name == 'latEq' and one.dtype == np.float64
    assert np.array_equal(one.coords['latitude'], np.linspace(-60, 60, NY))
    ds = cm.map_to_plane(np.arange(N, dtype=float), {'a': _vec(None, 'x'), 'b': _vec(None, 'y', time=t)}, dtype=np.float32)
    assert list(ds) == ['a', 'b'] and ds['b'].shape == (3, NY, NX) and ds['a'].dtype == np.float32 and ds['a'].name == 'a'
    a = [x for n, x in ctx.lib.args if n == 'xc_contour_map'][-1]
    assert a[7:10] == (N, 0, 2)                                      # 1-D levels are one set for all slabs
    _calls(ctx)
    for bad, text in ((lambda: cm.map_to_plane(ctr, _vec(None, 'v', n=N + 1, time=t)), 'along "contour"'),                    # wrong contour length
                      (lambda: cm.map_to_plane(ctr, {str(i): _vec(None, 'v') for i in range(9)}), 'one to 8 variables'),     # more than eight vectors
                      (lambda: cm.map_to_plane(ctr, {}), 'one to 8 variables'),
                      (lambda: cm.map_to_plane(ctr, _vec(None, 'v', time=np.arange(4.0))), 'leading dims'),                   # leading dims that do not match
                      (lambda: cm.map_to_plane(ctr, _vec(None, 'v', level=np.arange(3.0))), 'leading dims'),
                      (lambda: cm.map_to_plane(_vec(None, 'pv', time=np.arange(2.0)), _vec(None, 'v')), 'leading dims'),
                      (lambda: cm.map_to_plane(ctr, xa.DataArray(np.zeros(N), ('new',), {'new': np.arange(N)}, 'v')), '"contour" dim'),
                      (lambda: cm.map_to_plane(np.zeros((2, N)), _vec(None, 'v')), '1-D array'),
                      (lambda: cm.map_to_plane(ctr, [1.0, 2.0]), 'labelled array'),
                      (lambda: cm.map_to_plane(ctr, _vec(None, 'v'), dtype=np.int32), 'float32 or float64')):
        with pytest.raises(Exception) as e:
            bad()
        assert text in str(e.value), str(e.value)
    assert _calls(ctx) == []                                         # nothing reached the library
    # a tracer without leading dims takes vectors without them only
    flat = cm.tracer.isel({'time': 0})
    assert cm.map_to_plane(np.arange(N, dtype=float), _vec(None, 'v'), tracer=flat).shape == (NY, NX)
    with pytest.raises(Exception) as e:
        cm.map_to_plane(np.arange(N, dtype=float), _vec(None, 'v', time=t), tracer=flat)
    assert 'leading dims' in str(e.value)


def test_bare_array_entry(cm, ctx):
    q = np.zeros((NY, NX))
    p = xa.map_to_plane(q, np.arange(N, dtype=float), np.arange(N, dtype=float))
    assert type(p) is np.ndarray and p.shape == (NY, NX)
    ps = xa.map_to_plane(q[None].repeat(2, 0), np.arange(N, dtype=float), [np.arange(N, dtype=float)] * 2, dtype=np.float32)
    assert type(ps) is list and len(ps) == 2 and ps[0].shape == (2, NY, NX) and ps[0].dtype == np.float32
    assert _calls(ctx) == [('xc_contour_map', 1), ('xc_contour_map', 2)]
