# -*- coding: utf-8 -*-
"""K26 (xc_coarsen, xc_contour_lengths_scales) without a GPU: the restatement of its rule (cscale_ref.py) against values worked out
by hand; every deliberately wrong rule must disagree with it, in a bit of the plane or of a length (clength_ref.py on the coarse
planes), on the inputs the gpu tests run, so that none of those can pass vacuously; the binding's batching and refusals over the
stand-in library; and fractal_dimension."""
import numpy as np
import pytest

import clength_ref as L
import cscale_ref as R
import standin_lib
from standin_lib import RES, _Lib

import xcontour_amd as xa
from xcontour_amd import _native as nat
from xcontour_amd import utils

NAN, INF = np.nan, np.inf
F32, F64 = np.float32, np.float64


def _same(a, b):
    a, b = np.asarray(a, dtype=F64), np.asarray(b, dtype=F64)
    if a.shape != b.shape:
        return False
    return bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


# ---------------------------------------------------------------------------------------------------- the rule, by hand
def test_restatement_by_hand():
    q = np.array([[1.0, 2.0, 3.0, 4.0, 9.0],
                  [5.0, 6.0, 7.0, 8.0, 9.0],
                  [9.0, 9.0, 9.0, 9.0, 9.0]])
    assert _same(R.coarsen(q, 2), [[3.5, 5.5]])                      # trim: the third row and the fifth column fill no block
    assert _same(R.coarsen(q, 1), q) and R.coarsen(q.astype(F32), 1).dtype == F64
    assert R.coarsen(q, 3).shape == (1, 1) and R.coarsen(q[None, None], 2).shape == (1, 1, 1, 2)
    # the order: (a + b) + (c + d), rows from their first value.  1e16 + 1 = 1e16 in float64
    big = np.array([[1e16, 1.0], [-1e16, 1.0]])
    assert _same(R.coarsen(big, 2), [[((1e16 + 1.0) + (-1e16 + 1.0)) / 4.0]]) and R.coarsen(big, 2)[0, 0] == 0.0
    assert R.coarsen(big.T, 2)[0, 0] == 0.5                          # (1e16 - 1e16) + (1 + 1)
    # a sum starts FROM its first value: a block of -0.0 keeps its sign (0.0 + -0.0 would be +0.0)
    assert np.signbit(R.coarsen(np.full((2, 2), -0.0), 2)[0, 0]) and np.signbit(R.coarsen(np.full((2, 2), -0.0), 2, True)[0, 0])
    # NaN: the block is NaN, or the node is left out and the divisor is what was used
    n = np.array([[NAN, 2.0], [4.0, 9.0]])
    assert _same(R.coarsen(n, 2), [[NAN]]) and _same(R.coarsen(n, 2, True), [[15.0 / 3.0]])
    assert _same(R.coarsen(np.array([[NAN, NAN], [NAN, 7.0]]), 2, True), [[7.0]])              # the only node is the last one
    assert _same(R.coarsen(np.array([[NAN, NAN], [3.0, 7.0]]), 2, True), [[5.0]])              # a row without a node adds nothing
    assert _same(R.coarsen(np.full((2, 2), NAN), 2, True), [[NAN]])
    # an infinite node is an ordinary value in both modes
    i = np.array([[INF, 1.0], [1.0, 1.0]])
    assert _same(R.coarsen(i, 2), [[INF]]) and _same(R.coarsen(i, 2, True), [[INF]])
    assert _same(R.coarsen(np.array([[INF, 1.0], [-INF, 1.0]]), 2, True), [[NAN]])
    # a float32 tracer is promoted before anything is added
    f = np.array([[16777216.0, 1.0], [1.0, 1.0]], dtype=F32)
    assert R.coarsen(f, 2)[0, 0] == 16777219.0 / 4.0
    # coordinates: the same rule in one dimension, nothing cast
    assert _same(R.coarsen_coords([0.0, 1.0, 2.0, 3.0, 4.0], 2), [0.5, 2.5])
    assert _same(R.coarsen_coords([0.1, 0.2, 0.3], 3), [((0.1 + 0.2) + 0.3) / 3.0])


def test_refusals_restated():
    assert R.refusal(70, 530, [1, 2, 3, 5, 8]) == R.XC_OK
    assert R.refusal(70, 530, [0]) == R.refusal(70, 530, [65]) == R.refusal(70, 530, []) == R.refusal(70, 530, [1] * 9) == R.XC_EBADARG
    assert R.refusal(70, 530, [1] * 8) == R.XC_OK
    assert R.refusal(70, 530, [35]) == R.XC_OK and R.refusal(70, 530, [36]) == R.XC_EBADARG         # two coarse rows, one
    assert R.refusal(70, 530, [2], periodic=True) == R.XC_OK and R.refusal(70, 530, [3], periodic=True) == R.XC_EBADARG
    assert R.refusal(70, 10, [8]) == R.XC_EBADARG and R.refusal(70, 16, [8], periodic=True) == R.XC_OK   # one coarse column: a ring may have it
    assert R.refusal(70, 530, [64], lengths=False) == R.XC_OK and R.refusal(13, 37, [14], lengths=False) == R.XC_EBADARG


# ---------------------------------------------------------------------------------------------------- no case passes vacuously
GPU_PLANES = ((1, 13, 37), (2, 70, 530))
GPU_RATIOS = (2, 3, 5, 8, 64)


def _gpu_inputs():
    """(q, r) as the gpu record tests build them: both shapes with trimmed tails, both dtypes, specials set for the ratio"""
    for S, ny, nx in GPU_PLANES:
        for dtype in (F32, F64):
            for r in GPU_RATIOS:
                if ny // r >= 1 and nx // r >= 1:
                    yield R.with_specials(R.field(S, ny, nx, dtype, seed=r), r), r


def test_wrong_plane_rules_disagree_on_the_gpu_inputs():
    seen = padded = 0
    for q, r in _gpu_inputs():
        seen += 1
        for skipna in (False, True):
            ref = R.coarsen(q, r, skipna)
            assert not _same(R.wrong('pairwise', q, r, skipna), ref), ('pairwise', q.shape, q.dtype, r)
            assert not _same(R.wrong('column_first', q, r, skipna), ref), ('column_first', q.shape, q.dtype, r)
            if q.shape[-2] % r or q.shape[-1] % r:                    # (70 x 530 has no tail for 2 and 5; 13 x 37 has one for every ratio)
                padded += 1
                assert not _same(R.wrong('pad', q, r, skipna), ref), ('pad', q.shape, r)
        assert not _same(R.wrong('skipna_rr', q, r, True), R.coarsen(q, r, True)), ('skipna_rr', q.shape, r)
        # and the two NaN modes differ from one another
        assert not _same(R.coarsen(q, r, False), R.coarsen(q, r, True))
    assert seen == 2 * (4 + 5) and padded == 2 * 2 * (4 + 3)             # (13 x 37 has no block of 64)


def test_gpu_inputs_hold_what_they_promise():
    q = R.with_specials(R.field(1, 13, 37, F64, seed=2), 2)
    a, b = R.coarsen(q, 2, False)[0], R.coarsen(q, 2, True)[0]
    assert np.isnan(a[0, 0]) and np.isfinite(b[0, 0])                # NaN at a block's first node
    assert np.isnan(a[0, 1]) and np.isfinite(b[0, 1])                # ... at its last
    assert np.isnan(a[1, 0]) and b[1, 0] == q[0, 3, 1]               # the only node is the last: the mean is that node
    assert np.isnan(a[1, 2]) and b[1, 2] == q[0, 2, 4]               # the only node is the first
    assert np.isnan(a[1, 1]) and np.isfinite(b[1, 1])                # an all-NaN block row
    assert np.isnan(a[0, 2]) and np.isnan(b[0, 2])                   # an all-NaN block
    assert a[2, 0] == INF and b[2, 0] == INF and np.isnan(a[2, 1]) and np.isnan(b[2, 1])      # +inf; -inf + inf
    assert 13 % 2 and 37 % 2 and 70 % 3 and 530 % 3                  # tails in both directions


def test_wrong_rules_change_a_length():
    """the lengths K10's restatement gives on the coarse planes: every wrong coordinate rule moves at least one of them, and so do
    the plane rules that change more than the last bits of a node (pad, skipna over r * r).  The two wrong summation orders move
    nodes by an ulp or so, which a length need not show: they are caught in the plane itself (above)"""
    q = R.field(1, 29, 77, F64, seed=5)[0]
    y, x = R.coords(29, 1), R.coords(77, 2)
    for r in (2, 3):
        cq, cy, cx = R.coarsen(q, r), R.coarsen_coords(y, r), R.coarsen_coords(x, r)
        lev = R.levels(cq, 5)
        ref, cnt = L.contour_lengths(cq, lev, cy, cx)
        assert (cnt > 0).all()
        for kind in ('pad',):
            w = R.wrong(kind, q, r)
            wy = cy if w.shape[0] == cy.size else np.append(cy, 2 * cy[-1] - cy[-2])
            wx = cx if w.shape[1] == cx.size else np.append(cx, 2 * cx[-1] - cx[-2])
            assert not _same(L.contour_lengths(np.nan_to_num(w, nan=0.0), lev, wy, wx)[0], ref), kind
        for kind in R.WRONG_COORD:
            assert not _same(R.wrong_coords(kind, x, r), cx), kind
            assert not _same(L.contour_lengths(cq, lev, R.wrong_coords(kind, y, r), R.wrong_coords(kind, x, r))[0], ref), kind
    # skipna dividing by r * r, on a plane with NaN nodes
    qn = R.with_specials(q[None], 2)[0]
    cq = R.coarsen(qn, 2, True)
    lev = R.levels(cq, 5)
    ref = L.contour_lengths(cq, lev, R.coarsen_coords(y, 2), R.coarsen_coords(x, 2))[0]
    assert not _same(L.contour_lengths(R.wrong('skipna_rr', qn, 2, True), lev, R.coarsen_coords(y, 2), R.coarsen_coords(x, 2))[0], ref)


def test_exact_coordinates_make_the_user_identity():
    """coordinates 4.0 * arange: every block mean of ratio 1, 2, 4 is exact in float32, so a second float32 cast changes nothing --
    the ground of the facade test that compares with cal_contour_lengths(tracer=cm.coarsen(r))"""
    for n in (24, 48):
        c = 4.0 * np.arange(n)
        for r in (1, 2, 4):
            m = R.coarsen_coords(c, r)
            assert _same(m.astype(F32).astype(F64), m)
    assert not _same(R.coarsen_coords(R.coords(48, 2), 4).astype(F32).astype(F64), R.coarsen_coords(R.coords(48, 2), 4))


# ---------------------------------------------------------------------------------------------------- the binding, stand-in library
S, NY, NX, N = 5, 12, 16, 4


@pytest.fixture
def ctx(monkeypatch):
    for name in ('xc_coarsen', 'xc_coarsen_dev', 'xc_contour_lengths_scales', 'xc_contour_lengths_scales_dev'):
        monkeypatch.setitem(standin_lib._NSLAB_ARG, name, 3)
    c = nat.Context.__new__(nat.Context)
    c.lib, c.handle, c.device = _Lib(), None, 0
    c._buffers, c._resident, c._staged, c._ev_pool = [], {}, [], []
    c.max_batch_bytes = 8 << 30
    return c


def _calls(ctx):
    out, ctx.lib.calls = ctx.lib.calls, []
    return out


def _plane():
    return np.random.default_rng(7).standard_normal((S, NY, NX)), np.linspace(-1, 1, N), np.arange(NY, dtype=float), np.arange(NX, dtype=float)


def test_binding_limits_are_the_header_s():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'xcontour_hip.h')).read()
    assert int(re.search(r'#define XC_CSCALE_MAXR (\d+)', src).group(1)) == nat.XC_CSCALE_MAXR == R.MAXR
    assert int(re.search(r'#define XC_CSCALE_MAXRATIO (\d+)', src).group(1)) == nat.XC_CSCALE_MAXRATIO == R.MAXRATIO


def test_binding_batches_and_shapes(ctx):
    q, lev, y, x = _plane()
    lens, cnts = ctx.contour_lengths_scales(q, lev, y, x, [4, 1, 2])
    assert _calls(ctx) == [('xc_contour_lengths_scales', S)]
    assert lens.shape == cnts.shape == (3, S, N) and lens.dtype == F64 and cnts.dtype == np.uint64
    a = ctx.lib.args[-1][1]
    assert a[8:10] == (0.0, 0.0) and list(a[10]) == [4, 1, 2] and a[11:13] == (3, 0) and a[14:16] == (N, 0)
    ctx.max_batch_bytes = 2 * NY * NX * 8 + 8                        # the tracer alone counts: two slabs fit
    lens, _ = ctx.contour_lengths_scales(q, np.tile(lev, (S, 1)), y, x, [2, 2], radius=1.0, period=20.0, skipna=True)
    assert _calls(ctx) == [('xc_contour_lengths_scales', 2), ('xc_contour_lengths_scales', 2), ('xc_contour_lengths_scales', 1)]
    assert lens.shape == (2, S, N)                                   # the batches are joined along the slabs, ratio by ratio
    a = ctx.lib.args[-1][1]
    assert a[8:10] == (20.0, 1.0) and a[11:13] == (2, 1) and a[14:16] == (N, 1)
    out = ctx.coarsen(q, 3)
    assert out.shape == (S, NY // 3, NX // 3) and out.dtype == F64
    assert _calls(ctx) == [('xc_coarsen', 1)] * S                    # (the coarse plane is in the budget: one slab fits now)


def test_binding_resident_tracer_goes_to_the_dev_entries(ctx):
    q, lev, y, x = _plane()
    ctx._resident[q.ctypes.data] = q
    ctx.lib.resident_base = q.ctypes.data
    lens, cnts = ctx.contour_lengths_scales(q, lev, y, x, [1, 2])
    assert _calls(ctx) == [('xc_contour_lengths_scales_dev', S)]
    assert ctx.lib.args[-1][1][1] == RES and lens.shape == (2, S, N) and ctx._buffers == []
    assert ctx.coarsen(q, 2).shape == (S, NY // 2, NX // 2)
    assert _calls(ctx) == [('xc_coarsen_dev', S)] and ctx._buffers == []
    # the device form trusts its caller: the binding checks levels and coordinates as the host form does, with its codes
    with pytest.raises(nat.XContourHipError) as e:
        ctx.contour_lengths_scales(q, lev[::-1], y, x, [2])
    assert e.value.code == nat.XC_EEDGES
    with pytest.raises(nat.XContourHipError) as e:
        ctx.contour_lengths_scales(q, lev, np.where(y == 3, INF, y), x, [2])
    assert e.value.code == nat.XC_EBADARG


def test_binding_refuses_what_the_library_would(ctx):
    q, lev, y, x = _plane()
    cl = ctx.contour_lengths_scales
    for bad, text in ((lambda: cl(q, lev, y, x, [0]), 'ratio 0'), (lambda: cl(q, lev, y, x, [2, 65]), 'ratio 65'),
                      (lambda: cl(q, lev, y, x, []), 'ratios'), (lambda: cl(q, lev, y, x, [1] * 9), 'ratios'),
                      (lambda: cl(q, lev, y, x, [2, 7]), 'ratio 7'),                          # 12 // 7 = 1 coarse row
                      (lambda: cl(q[:, :, :10], lev, y, x[:10], [6]), 'ratio 6'),             # one coarse column of a plain plane
                      (lambda: cl(q, lev, y, x, [2, 3], period=16.0), 'ratio 3'),             # 16 % 3 != 0 on a ring
                      (lambda: cl(q, lev, y, x, [2], period=15.0), 'period'),                 # K10's condition: not longer than the span
                      (lambda: cl(q, lev, y[:-1], x, [2]), 'coordinates'), (lambda: cl(q[0], lev, y, x, [2]), 'nslab'),
                      (lambda: ctx.coarsen(q, 0), 'ratio 0'), (lambda: ctx.coarsen(q, 65), 'ratio 65'),
                      (lambda: ctx.coarsen(q, 13), 'ratio 13')):
        with pytest.raises(nat.XContourHipError) as e:
            bad()
        assert e.value.code == nat.XC_EBADARG and text in str(e.value), str(e.value)
    assert _calls(ctx) == []
    for ratios, period, ny, nx in (([0], None, NY, NX), ([7], None, NY, NX), ([3], 16.0, NY, NX), ([6], None, NY, 10), ([8], 16.0, 16, NX)):
        ok = R.refusal(ny, nx, ratios, periodic=period is not None) == R.XC_OK       # the restatement refuses the same calls
        assert ok == (ratios == [8])
    cl(q, lev, y, x, [6]); cl(q, lev, y, x, [4], period=16.0); ctx.coarsen(q, 12)
    assert len(_calls(ctx)) == 3


# ---------------------------------------------------------------------------------------------------- the facade, stand-in library
@pytest.fixture
def cm(ctx, monkeypatch):
    monkeypatch.setattr(nat, 'default_context', lambda device=0: ctx)
    monkeypatch.setattr(xa, 'default_context', lambda device=0: ctx)
    lat, lon, t = np.linspace(-60, 60, NY), np.linspace(0, 337.5, NX), np.arange(3.0)
    q = np.random.default_rng(3).standard_normal((3, NY, NX))
    tr = xa.DataArray(q, ('time', 'latitude', 'longitude'), {'time': t, 'latitude': lat, 'longitude': lon}, 'pv')
    return xa.Contour2D(tr, np.ones((NY, NX)), dims={'X': 'longitude', 'Y': 'latitude'}, dimEq={'Y': 'latitude'}, increase=True, lt=True)


def test_facade_shapes_chunks_and_coords(cm, ctx):
    lev = np.array([0.5, -0.5, NAN, 0.0])
    out = cm.cal_contour_lengths_coarsened(lev, [1, 2, 4], latlon=True, periodic=True)
    assert _calls(ctx) == [('xc_contour_lengths_scales', 3)]
    assert type(out) is list and len(out) == 3 and all(o.dims == ('time', 'contour') and o.shape == (3, 4) and o.dtype == cm.dtype for o in out)
    a = ctx.lib.args[-1][1]
    assert a[8] == float(np.deg2rad(np.float32(360.0))) and a[9] == xa.Rearth and list(a[10]) == [1, 2, 4] and a[12] == 0
    one = cm.cal_contour_lengths_coarsened(lev, 2, skipna=True)
    assert one.shape == (3, 4) and ctx.lib.args[-1][1][12] == 1 and _calls(ctx) == [('xc_contour_lengths_scales', 3)]
    ten = cm.cal_contour_lengths_coarsened(lev, [1, 2, 3, 4, 6, 1, 2, 3, 4, 6])
    assert len(ten) == 10 and _calls(ctx) == [('xc_contour_lengths_scales', 3)] * 2
    assert [list(x[10]) for n, x in ctx.lib.args[-2:]] == [[1, 2, 3, 4, 6, 1, 2, 3], [4, 6]]
    for bad in (lambda: cm.cal_contour_lengths_coarsened(lev, []), lambda: cm.cal_contour_lengths_coarsened(lev, [0]),
                lambda: cm.cal_contour_lengths_coarsened(lev, [65])):
        with pytest.raises(Exception) as e:
            bad()
        assert 'ratios' in str(e.value)
    c = cm.coarsen(3)
    assert c.dims == ('time', 'latitude', 'longitude') and c.shape == (3, 4, 5) and c.dtype == F64 and c.name == 'pv'
    assert _same(c.coords['latitude'], R.coarsen_coords(np.linspace(-60, 60, NY), 3)) and np.array_equal(c.coords['time'], np.arange(3.0))
    assert _same(c.coords['longitude'], R.coarsen_coords(np.linspace(0, 337.5, NX), 3))
    d = xa.coarsen(cm.tracer.isel({'time': 0}).transpose('longitude', 'latitude'), ('latitude', 'longitude'), 2, skipna=True)
    assert d.dims == ('longitude', 'latitude') and d.shape == (8, 6)


# ---------------------------------------------------------------------------------------------------- fractal_dimension
def test_fit_slope_is_exact_on_representable_points():
    x = np.arange(4.0)
    assert utils._fit_slope(x, 1.5 * x + 2.0) == 1.5
    assert utils._fit_slope(-x, 1.5 * x + 2.0) == -1.5
    y = np.stack([0.5 * x, -2.0 * x + 1.0, np.full(4, 3.0)], axis=1)
    assert np.array_equal(utils._fit_slope(x[:, None], y, axis=0), [0.5, -2.0, 0.0])
    assert np.array_equal(utils._fit_slope(x[None, :], y.T, axis=1), [0.5, -2.0, 0.0])


def test_fractal_dimension_and_its_nan_rules():
    rulers = np.array([1.0, 2.0, 4.0, 8.0])
    for D in (1.0, 1.25, 2.0):
        lengths = 100.0 * rulers ** (1.0 - D)                        # counts = lengths / rulers ~ rulers ** -D
        assert abs(xa.fractal_dimension(lengths, rulers) - D) < 1e-12
    stack = np.stack([100.0 * rulers ** -0.5, 3.0 * rulers ** 0.0, 7.0 * rulers ** -1.0], axis=1)
    assert np.allclose(xa.fractal_dimension(stack, rulers), [1.5, 1.0, 2.0], rtol=0, atol=1e-12)
    assert np.allclose(xa.fractal_dimension(stack.T, rulers, axis=1), [1.5, 1.0, 2.0], rtol=0, atol=1e-12)
    assert np.allclose(xa.fractal_dimension(stack, rulers[:, None] * np.ones((1, 3))), [1.5, 1.0, 2.0], rtol=0, atol=1e-12)
    bad = stack.copy()
    bad[1, 0], bad[2, 1] = NAN, 0.0
    d = xa.fractal_dimension(bad, rulers)
    assert np.isnan(d[0]) and np.isnan(d[1]) and abs(d[2] - 2.0) < 1e-12
    bad[3, 2] = -1.0
    assert np.isnan(xa.fractal_dimension(bad, rulers)).all()
    assert np.isnan(xa.fractal_dimension(stack, [1.0, 2.0, 0.0, 8.0])).all() and np.isnan(xa.fractal_dimension(stack, [1.0, NAN, 4.0, 8.0])).all()
