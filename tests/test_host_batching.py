# -*- coding: utf-8 -*-
"""How `_native.Context` cuts a stack into batches, pinned without a GPU: a Context over a stand-in library that records
(entry point, nslab) per call.  The batch boundaries, the order of the library calls, the container shape of every joined result
and the reads of a lazy stack (every slab once, in order) are what a change to the batching must leave alone."""
import numpy as np
import pytest

from standin_lib import RES, _K12, _Lib

from xcontour_amd import _native as nat
from xcontour_amd import labeled as lb

S, NY, NX, N = 5, 6, 8, 4
SLAB = NY * NX * 8                      # bytes of one float64 slab


@pytest.fixture
def ctx():
    c = nat.Context.__new__(nat.Context)
    c.lib, c.handle, c.device = _Lib(), None, 0
    c._buffers, c._resident, c._staged, c._ev_pool = [], {}, [], []
    c.max_batch_bytes = 2 * SLAB + 8
    return c


@pytest.fixture
def q():
    return np.random.default_rng(7).standard_normal((S, NY, NX))


def _calls(ctx):
    out, ctx.lib.calls = ctx.lib.calls, []
    return out


def _seq(name, *ns):
    return [(name, n) for n in ns]


def test_minmax_and_contours_batches(ctx, q):
    mm = ctx.minmax(q)
    assert _calls(ctx) == _seq('xc_minmax', 2, 2, 1)
    assert type(mm) is np.ndarray and mm.shape == (S, 2) and mm.dtype == np.float64
    ctr = ctx.contours(q, N, True, np.float32)
    assert _calls(ctx) == _seq('xc_minmax', 2, 2, 1) + _seq('xc_levels', S)
    assert type(ctr) is np.ndarray and ctr.shape == (S, N)
    res = ctx.contours(q, N, True, np.float32, want_minmax=True)
    assert _calls(ctx) == _seq('xc_minmax', 2, 2, 1) + _seq('xc_levels', S)
    assert type(res) is tuple and res[0].shape == (S, N) and res[1].shape == (S, 2)
    ctx.max_batch_bytes = 8 << 30                                   # everything fits: the one-call form
    res = ctx.contours(q, N, True, np.float32, want_minmax=True)
    assert _calls(ctx) == _seq('xc_contours', S)
    assert type(res) is tuple and res[0].shape == (S, N) and res[1].shape == (S, 2)


def test_hist_batches(ctx, q):
    edges = np.linspace(-3, 3, N + 1)
    out = ctx.hist(q, edges)
    assert _calls(ctx) == _seq('xc_hist', 2, 2, 1)
    assert type(out) is dict and list(out) == ['pdf', 'cdf', 'counts']
    assert out['pdf'].shape == out['cdf'].shape == (S, 1, N) and out['counts'].shape == (S, N) and out['counts'].dtype == np.uint64
    # per-slab edges, per-slab weights and one integrand: 3 x 8 bytes per cell staged, one slab per batch
    out = ctx.hist(q, np.tile(edges, (S, 1)), dA=np.ones((S, NY, NX)), integrands=[q * 2.0], want=('cdf',))
    assert _calls(ctx) == _seq('xc_hist', 1, 1, 1, 1, 1)
    assert type(out) is dict and list(out) == ['cdf'] and out['cdf'].shape == (S, 2, N)


def test_grad2_batches(ctx, q):
    g = ctx.grad2(q, np.ones(NY), np.ones(NY))
    assert _calls(ctx) == _seq('xc_grad2', 1, 1, 1, 1, 1)          # tracer + the float64 result: 2 x 8 bytes per cell
    assert type(g) is np.ndarray and g.shape == (S, NY, NX) and g.dtype == np.float64


def test_crossing_batches(ctx, q):
    levels = np.linspace(-1, 1, N)
    res = ctx.crossing(q, levels, np.ones((NY, NX)))
    assert _calls(ctx) == _seq('xc_crossing', 2, 2, 1)
    assert type(res) is tuple and len(res) == 2
    assert res[0].shape == res[1].shape == (S, N) and res[0].dtype == np.float64 and res[1].dtype == np.uint64
    # several strides: both strides of a batch on its one upload, before the next batch
    res = ctx.crossing(q, np.tile(levels, (S, 1)), np.ones((NY, NX)), stride=[1, 2])
    assert _calls(ctx) == _seq('xc_crossing_dev', 2, 2, 2, 2, 1, 1)
    assert type(res) is list and len(res) == 2
    for r in res:
        assert type(r) is tuple and r[0].shape == r[1].shape == (S, N) and r[0].dtype == np.float64 and r[1].dtype == np.uint64
    assert ctx._buffers == []                                       # the temporaries of every batch were freed


def test_contour_lengths_batches(ctx, q):
    res = ctx.contour_lengths(q, np.linspace(-1, 1, N), np.arange(NY, dtype=float), np.arange(NX, dtype=float))
    assert _calls(ctx) == _seq('xc_contour_lengths', 2, 2, 1)
    assert type(res) is tuple and len(res) == 2
    assert res[0].shape == res[1].shape == (S, N) and res[0].dtype == np.float64 and res[1].dtype == np.uint64


def test_lwa_batches(ctx, q):
    Q = np.sort(q[:, :, 0], axis=1)
    out, masks = ctx.lwa(q, Q, np.arange(NY, dtype=float), np.ones(NY), 1.0)
    assert _calls(ctx) == _seq('xc_lwa', 1, 1, 1, 1, 1)            # tracer + the float64 result
    assert out.shape == (S, NY, NX) and out.dtype == np.float64 and masks is None
    out, masks = ctx.lwa(q, Q, np.arange(NY, dtype=float), np.ones((NY, NX)), 1.0, M=np.ones(NY), mask_idx=[1, 3], exact=False)
    assert _calls(ctx) == _seq('xc_lwa', 1, 1, 1, 1, 1)
    assert out.shape == (S, NY, NX) and masks.shape == (S, 2, NY, NX) and masks.dtype == np.int8


def test_sort_profile_batches(ctx, q):
    ctx.max_batch_bytes = 2 * NY * NX * 40 + 8                      # tracer + the sort's four work arrays: 40 bytes per cell
    out = ctx.sort_profile(q, dA=np.ones(NY), targets=np.array([0.5, 1.5, 2.5]), tbl=np.arange(NY, dtype=float),
                           coord=np.arange(NY, dtype=float))
    assert _calls(ctx) == _seq('xc_sort_profile_batch', 2, 2, 1)
    assert type(out) is dict and list(out) == ['nvalid', 'Q', 'bpe']
    assert out['nvalid'].shape == (S,) and out['nvalid'].dtype == np.int64 and out['Q'].shape == (S, 3) and out['bpe'].shape == (S,)
    ctx.max_batch_bytes = 2 * NY * NX * 72 + 8                      # + both full-length outputs, a per-slab mask and per-slab weights
    out = ctx.sort_profile(q, dA=np.ones((S, NY, NX)), mask=np.ones((S, NY, NX)), want_sorted=True, want_acum=True)
    assert _calls(ctx) == _seq('xc_sort_profile_batch', 2, 2, 1)
    assert list(out) == ['nvalid', 'q_sorted', 'acum'] and out['q_sorted'].shape == out['acum'].shape == (S, NY * NX)
    # one plane in, scalars / 1-D arrays out
    out = ctx.sort_profile(q[0], targets=np.array([0.5, 1.5]), tbl=np.arange(NY, dtype=float), coord=np.arange(NY, dtype=float),
                           want_sorted=True)
    assert _calls(ctx) == _seq('xc_sort_profile_batch', 1)
    assert type(out['nvalid']) is int and type(out['bpe']) is float and out['Q'].shape == (2,) and out['q_sorted'].shape == (NY * NX,)


class _Source(object):
    """a lazy (S, ny, nx) source that records which slabs every read asks for"""

    def __init__(self, a):
        self.a, self.shape, self.dtype, self.reads = a, a.shape, a.dtype, []

    def __getitem__(self, key):
        self.reads.append(tuple(range(*key[0].indices(self.shape[0]))))
        return self.a[key]


def _lazy(q):
    src = _Source(q)
    return src, lb.LazyStack(src, [0], 1, 2)


@pytest.mark.parametrize('method', ['minmax', 'contours', 'hist', 'grad2', 'crossing', 'crossing_strides', 'contour_lengths', 'lwa',
                                    'contour_segments', 'contour_pieces', 'local_contour_lengths', 'sort_profile'])
def test_a_lazy_stack_is_read_batch_by_batch_every_slab_once_in_order(ctx, q, method):
    src, st = _lazy(q)
    levels = np.linspace(-1, 1, N)
    one_by_one = [(0,), (1,), (2,), (3,), (4,)]
    pairs = [(0, 1), (2, 3), (4,)]
    if method == 'minmax':
        out, want = ctx.minmax(st), pairs
    elif method == 'contours':
        out, want = ctx.contours(st, N, True, np.float64), pairs
    elif method == 'hist':
        src2, st2 = _lazy(q * 2.0)
        out, want = ctx.hist(st, np.linspace(-3, 3, N + 1), integrands=[st2], want=('cdf',))['cdf'], one_by_one
        assert src2.reads == want                                   # the lazy integrand too
    elif method == 'grad2':
        out, want = ctx.grad2(st, np.ones(NY), np.ones(NY)), one_by_one
    elif method == 'crossing':
        out, want = ctx.crossing(st, levels, np.ones((NY, NX)))[0], pairs
    elif method == 'crossing_strides':
        out, want = ctx.crossing(st, levels, np.ones((NY, NX)), stride=[1, 2])[1][0], pairs
    elif method == 'contour_lengths':
        out, want = ctx.contour_lengths(st, levels, np.arange(NY, dtype=float), np.arange(NX, dtype=float))[0], pairs
    elif method == 'contour_segments':
        out, want = ctx.contour_segments(st, levels)[0], pairs
    elif method == 'contour_pieces':
        out, want = ctx.contour_pieces(st, levels, np.arange(NY, dtype=float), np.arange(NX, dtype=float))[0], pairs
    elif method == 'local_contour_lengths':
        ctx.max_batch_bytes = 2 * (SLAB + 4 * NWY * NWX * 8) + 8
        out, want = ctx.local_contour_lengths(st, np.arange(NY, dtype=float), np.arange(NX, dtype=float), WIN, STR, 4)[0], pairs
    elif method == 'lwa':
        out, want = ctx.lwa(st, np.sort(q[:, :, 0], axis=1), np.arange(NY, dtype=float), np.ones(NY), 1.0)[0], one_by_one
    else:
        ctx.max_batch_bytes = 2 * NY * NX * 40 + 8
        out, want = ctx.sort_profile(st, targets=np.array([0.5]))['Q'], pairs
    assert src.reads == want
    assert out.shape[0] == S
    # everything in one batch: one read of the whole stack
    src.reads[:] = []
    ctx.max_batch_bytes = 8 << 30
    ctx.minmax(st)
    assert src.reads == [tuple(range(S))]


# ------------------------------------------------------------------ the contour family (K10 periodic, K11, K12, K13)
Y, X = np.arange(NY, dtype=float), np.arange(NX, dtype=float)
PERIOD, RADIUS = float(NX), 2.5
WIN, STR = (3, 4), (2, 3)                                           # K11: windows of 3 x 4 nodes every 2 rows / 3 columns
NWY, NWX = 3, 3                                                     # ceil(6 / 2), ceil(8 / 3)
OB = NWY * NWX * 8                                                  # bytes of one slab's windows in one K11 output
BATCHES = [(0, 2), (2, 2), (4, 1)]                                  # (first slab, slabs) of the batches of S = 5
F64 = nat.XC_F64


def _per_slab_levels():
    return np.linspace(-1, 1, N)[None, :] + 0.01 * np.arange(S)[:, None]


def _make_resident(ctx, q):
    """what keep_resident(q) leaves behind: batch [s0, s1) of `q` has its mirror at RES + s0 * SLAB"""
    ctx._resident[q.ctypes.data] = q
    ctx.lib.resident_base = q.ctypes.data


def _take(ctx):
    """(calls, args, mallocs, the address of every allocation) since the last _take"""
    lib = ctx.lib
    out = lib.calls, [a for _, a in lib.args], lib.mallocs
    addr, at = [], lib._base
    for n in lib.mallocs:
        addr.append(at)
        at += (n + 4095) & ~4095
    lib._base = at
    lib.calls, lib.args, lib.mallocs = [], [], []
    return out + (addr,)


def _where_q(q, resident, s0):
    return (RES if resident else q.ctypes.data) + s0 * SLAB


@pytest.mark.parametrize('period', [None, PERIOD])
def test_contour_lengths_host_path_plain_and_periodic(ctx, q, period):
    res = ctx.contour_lengths(q, np.linspace(-1, 1, N), Y, X, radius=RADIUS, period=period)
    calls, args, mallocs, _ = _take(ctx)
    name = 'xc_contour_lengths' if period is None else 'xc_contour_lengths_periodic'
    assert calls == _seq(name, 2, 2, 1) and mallocs == []
    mid = (RADIUS,) if period is None else (PERIOD, RADIUS)         # the period goes between xcoord and the radius
    for a, (s0, n) in zip(args, BATCHES):
        assert a[:8] + a[8:8 + len(mid)] == (None, q.ctypes.data + s0 * SLAB, F64, n, NY, NX, Y.ctypes.data, X.ctypes.data) + mid
        assert a[9 + len(mid):11 + len(mid)] == (N, 0) and len(a) == 13 + len(mid)
        assert all(type(v) is float for v in a[8:8 + len(mid)])
    assert type(res) is tuple and len(res) == 2
    assert res[0].shape == res[1].shape == (S, N) and res[0].dtype == np.float64 and res[1].dtype == np.uint64
    assert ctx._buffers == []


@pytest.mark.parametrize('period', [None, PERIOD])
def test_contour_lengths_resident_path_plain_and_periodic(ctx, q, period):
    _make_resident(ctx, q)
    res = ctx.contour_lengths(q, _per_slab_levels(), Y, X, radius=RADIUS, period=period)
    calls, args, mallocs, at = _take(ctx)
    name = 'xc_contour_lengths_dev' if period is None else 'xc_contour_lengths_periodic_dev'
    assert calls == _seq(name, 2, 2, 1)
    assert mallocs == [b for _, n in BATCHES for b in (NY * 8, NX * 8, n * N * 8, n * N * 8, n * N * 8)]
    mid = (RADIUS,) if period is None else (PERIOD, RADIUS)
    for k, (a, (s0, n)) in enumerate(zip(args, BATCHES)):
        dy, dx, dc, dl, dn = at[5 * k:5 * k + 5]
        assert a == (None, RES + s0 * SLAB, F64, n, NY, NX, dy, dx) + mid + (dc, N, 1, dl, dn)
    assert type(res) is tuple and len(res) == 2
    assert res[0].shape == res[1].shape == (S, N) and res[0].dtype == np.float64 and res[1].dtype == np.uint64
    assert ctx._buffers == []


def _twos_but_in_the_second_batch(lib):
    """for _Lib.d2h_u64: every count is 2, but 0 in the second batch -- the batches are told apart by K12's count-only calls"""
    return 0 if sum(1 for name, a in lib.args if name in _K12 and a[9] == 0) == 2 else 2


@pytest.mark.parametrize('resident', [False, True])
@pytest.mark.parametrize('periodic', [False, True])
def test_contour_segments_two_passes_per_batch(ctx, q, periodic, resident):
    if resident:
        _make_resident(ctx, q)
    ctx.lib.d2h_u64 = _twos_but_in_the_second_batch
    res = ctx.contour_segments(q, _per_slab_levels(), periodic=periodic)
    calls, args, mallocs, at = _take(ctx)
    name = _K12[1] if periodic else _K12[0]
    assert calls == _seq(name, 2, 2, 2, 1, 1)                       # count and records; count alone (total 0); count and records
    want_m, want_a, k = [], [], 0
    for b, (s0, n) in enumerate(BATCHES):
        total = 0 if b == 1 else 2 * n * N
        stage = ([] if resident else [n * SLAB]) + [n * N * 8, n * N * 8]            # [tracer,] contours, counts
        recs = [total * 8, total * 8, total * 32] if total else []
        want_m += stage + recs
        dc, dn = at[k + len(stage) - 2], at[k + len(stage) - 1]
        head = (None, RES + s0 * SLAB if resident else at[k], F64, n, NY, NX, dc, N, 1)
        want_a.append(head + (0, dn, None, None, None))
        if total:
            want_a.append(head + (total, dn) + tuple(at[k + len(stage):k + len(stage) + 3]))
        k += len(stage) + len(recs)
    assert mallocs == want_m and args == want_a
    cnt, ef, et, pts = res
    assert type(res) is tuple and len(res) == 4
    assert cnt.shape == (S, N) and cnt.dtype == np.uint64 and cnt[:, 0].tolist() == [2, 2, 0, 0, 2]
    assert ef.shape == et.shape == (24,) and ef.dtype == et.dtype == np.int64
    assert pts.shape == (24, 4) and pts.dtype == np.float64
    assert ctx._buffers == []
    # levels every slab shares: uploaded whole with every batch, the per-slab flag 0; everything zero: one pass, empty records
    ctx.lib.d2h_u64 = None
    res = ctx.contour_segments(q, np.linspace(-1, 1, N), periodic=periodic)
    calls, args, mallocs, at = _take(ctx)
    assert calls == _seq(name, 2, 2, 1) and all(a[7:10] == (N, 0, 0) for a in args)
    assert mallocs == [b for _, n in BATCHES for b in ([] if resident else [n * SLAB]) + [N * 8, n * N * 8]]
    assert res[0].shape == (S, N) and not res[0].any() and res[0].dtype == np.uint64
    assert res[1].shape == res[2].shape == (0,) and res[1].dtype == res[2].dtype == np.int64
    assert res[3].shape == (0, 4) and res[3].dtype == np.float64
    assert ctx._buffers == []


@pytest.mark.parametrize('resident', [False, True])
@pytest.mark.parametrize('period', [None, PERIOD])
def test_contour_pieces_runs_k13_on_the_records_of_each_batch(ctx, q, period, resident):
    if resident:
        _make_resident(ctx, q)
    ctx.lib.d2h_u64 = _twos_but_in_the_second_batch
    res = ctx.contour_pieces(q, _per_slab_levels(), Y, X, radius=RADIUS, period=period)
    calls, args, mallocs, at = _take(ctx)
    seg = _K12[0] if period is None else _K12[1]
    K13 = 'xc_contour_pieces_dev'
    assert calls == [(seg, 2), (seg, 2), (K13, 2 * N), (seg, 2), (seg, 1), (seg, 1), (K13, N)]
    want_m, want_a, k = [], [], 0
    for b, (s0, n) in enumerate(BATCHES):
        total = 0 if b == 1 else 2 * n * N
        stage = ([] if resident else [n * SLAB]) + [n * N * 8, NY * 8, NX * 8, n * N * 8, n * N * 8]
        recs = [total * 8, total * 8, total * 32, total * 56] if total else []
        want_m += stage + recs
        dc, dy, dx, dn, dpc = at[k + len(stage) - 5:k + len(stage)]
        head = (None, RES + s0 * SLAB if resident else at[k], F64, n, NY, NX, dc, N, 1)
        want_a.append(head + (0, dn, None, None, None))
        if total:
            df, dto, dp, drec = at[k + len(stage):k + len(stage) + 4]
            want_a.append(head + (total, dn, df, dto, dp))
            col = [drec + c * total * 8 for c in range(6)]
            want_a.append((None, n * N, dn, df, dto, dp, NY, NX) + ((0, dy, dx, 0.0) if period is None else (1, dy, dx, PERIOD))
                          + (RADIUS, total, dpc, col[0], col[1], drec + 48 * total, drec + 52 * total, col[2], col[3], col[4], col[5]))
        k += len(stage) + len(recs)
    assert mallocs == want_m and args == want_a
    pc, tab = res
    assert type(res) is tuple and len(res) == 2
    assert pc.shape == (S, N) and pc.dtype == np.uint64 and pc[:, 0].tolist() == [2, 2, 0, 0, 2]
    assert type(tab) is np.ndarray and tab.shape == (24,) and tab.dtype == nat.Context.PIECE_DTYPE
    assert ctx._buffers == []
    ctx.lib.d2h_u64 = None                                          # everything zero: K13 is never run
    pc, tab = ctx.contour_pieces(q, np.linspace(-1, 1, N), Y, X, period=period)
    calls, args, mallocs, at = _take(ctx)
    assert calls == _seq(seg, 2, 2, 1) and all(a[7:10] == (N, 0, 0) for a in args)
    assert mallocs == [b for _, n in BATCHES for b in ([] if resident else [n * SLAB]) + [N * 8, NY * 8, NX * 8, n * N * 8, n * N * 8]]
    assert pc.shape == (S, N) and pc.dtype == np.uint64 and not pc.any()
    assert tab.shape == (0,) and tab.dtype == nat.Context.PIECE_DTYPE
    assert ctx._buffers == []


@pytest.mark.parametrize('with_levels', [False, True])
@pytest.mark.parametrize('resident', [False, True])
@pytest.mark.parametrize('period', [None, PERIOD])
def test_local_contour_lengths_batches(ctx, q, period, resident, with_levels):
    """a slab of K11 stages the tracer and four window arrays: the cap that gives batches of 2, 2, 1 is its own"""
    ctx.max_batch_bytes = 2 * (SLAB + 4 * OB) + 8
    if resident:
        _make_resident(ctx, q)
    levels = np.linspace(-1, 1, S * NWY * NWX).reshape(S, NWY, NWX) if with_levels else None
    res = ctx.local_contour_lengths(q, Y, X, WIN, STR, 5, levels=levels, radius=RADIUS, period=period)
    calls, args, mallocs, at = _take(ctx)
    name = 'xc_local_contour_lengths' + ('' if period is None else '_periodic') + ('_dev' if resident else '')
    assert calls == _seq(name, 2, 2, 1)
    rest = (() if period is None else (PERIOD,)) + (RADIUS, 3, 4, 2, 3, 5)           # the period goes between xcoord and the radius
    if resident:
        assert mallocs == [b for _, n in BATCHES for b in [NY * 8, NX * 8] + ([n * OB] if with_levels else []) + [n * OB] * 3]
        per = 6 if with_levels else 5
        for k, (a, (s0, n)) in enumerate(zip(args, BATCHES)):
            b = at[per * k:per * k + per]
            assert a == (None, RES + s0 * SLAB, F64, n, NY, NX, b[0], b[1]) + rest + (b[2] if with_levels else None,) + tuple(b[-3:])
    else:
        assert mallocs == []
        for a, (s0, n) in zip(args, BATCHES):
            assert a[:8 + len(rest)] == (None, q.ctypes.data + s0 * SLAB, F64, n, NY, NX, Y.ctypes.data, X.ctypes.data) + rest
            assert a[8 + len(rest)] == (levels.ctypes.data + s0 * OB if with_levels else None) and len(a) == 12 + len(rest)
    assert type(res) is tuple and len(res) == 3
    assert res[0].shape == res[1].shape == res[2].shape == (S, NWY, NWX)
    assert res[0].dtype == res[1].dtype == np.float64 and res[2].dtype == np.uint64
    assert ctx._buffers == []


# ------------------------------------------------------------------ what the four methods refuse, and in which words
def _call(ctx, method, q, contours=None, y=Y, x=X, period=None, window=WIN, stride=STR, levels=None):
    if contours is None:
        contours = np.linspace(-1, 1, N)
    if method == 'contour_lengths':
        return ctx.contour_lengths(q, contours, y, x, period=period)
    if method == 'contour_segments':
        return ctx.contour_segments(q, contours, periodic=period is not None)
    if method == 'contour_pieces':
        return ctx.contour_pieces(q, contours, y, x, period=period)
    return ctx.local_contour_lengths(q, y, x, window, stride, 4, levels=levels, period=period)


K10, K11, K12, K13 = 'contour_lengths', 'local_contour_lengths', 'contour_segments', 'contour_pieces'
_BAD, _EDGES = nat.XC_EBADARG, nat.XC_EEDGES
_Q_TEXT = 'q must be (nslab, ny, nx)'
_C_TEXT = 'contours must be (N,) or (nslab, N)'
_ASC = '%s: contours must be ascending without NaN'
_LEN = '%%s: coordinates of length (%%d, %%d) for a (%d, %d) plane' % (NY, NX)
_FIN = '%s: coordinates must be finite'
_PER = ('%s: period must be finite, non-zero, of the sign of xcoord[nx-1] - xcoord[0] and longer than that span, and nx >= 2')
_XNAN = np.where(np.arange(NX) == 3, np.nan, X)
_YINF = np.where(np.arange(NY) == 2, np.inf, Y)
# (method, what is wrong, keyword arguments of _call, error code, text); 'resident': the tracer has a device mirror
_REFUSED = [(m, 'q not 3-D', dict(q=np.zeros((NY, NX))), _BAD, _Q_TEXT) for m in (K10, K11, K12, K13)]
for m, who in ((K10, 'xc_contour_lengths'), (K12, 'xc_contour_segments'), (K13, 'xc_contour_pieces')):
    res = dict(resident=True) if m == K10 else {}                   # K10's host path leaves these two to the C library, same texts
    _REFUSED += [(m, 'contours 3-D', dict(contours=np.zeros((S, 1, N))), _BAD, _C_TEXT),
                 (m, 'wrong leading contour dim', dict(contours=np.zeros((S + 1, N))), _BAD, _C_TEXT),
                 (m, 'zero contours', dict(contours=np.zeros(0)), _BAD, _C_TEXT),
                 (m, 'a NaN contour', dict(contours=np.array([0.0, np.nan, 1.0]), **res), _EDGES, _ASC % who),
                 (m, 'a descending contour', dict(contours=np.array([0.0, 1.0, 0.5]), **res), _EDGES, _ASC % who),
                 (m, 'a descending contour of one slab', dict(contours=np.where(np.arange(S)[:, None] == 0, -1.0, 1.0)
                                                               * np.arange(3.0), **res), _EDGES, _ASC % who)]
for m, who, pwho in ((K10, 'xc_contour_lengths', 'xc_contour_lengths_periodic'), (K13, 'xc_contour_pieces', 'xc_contour_pieces'),
                     (K11, 'xc_local_contour_lengths', 'xc_local_contour_lengths_periodic')):
    res = dict(resident=True) if m == K10 else {}                   # without a period K10's host path leaves finiteness to C too
    _REFUSED += [(m, 'wrong ycoord length', dict(y=np.arange(NY + 1.0)), _BAD, _LEN % (who, NY + 1, NX)),
                 (m, 'wrong xcoord length', dict(x=np.arange(NX - 1.0)), _BAD, _LEN % (who, NY, NX - 1)),
                 (m, 'xcoord 2-D', dict(x=np.zeros((1, NX))), _BAD, _LEN % (who, NY, NX)),
                 (m, 'a NaN xcoord', dict(x=_XNAN, **res), _BAD, _FIN % who),
                 (m, 'an infinite ycoord', dict(y=_YINF, **res), _BAD, _FIN % who),
                 (m, 'a NaN xcoord, periodic', dict(x=_XNAN, period=PERIOD), _BAD, _FIN % who),
                 (m, 'nx == 1 with a period', dict(q=np.zeros((S, NY, 1)), x=np.zeros(1), period=1.0), _BAD, _PER % pwho)]
    # tests/test_gpu_periodic_contour_lengths.py::test_bad_periods_rejected, for a span of NX - 1
    _REFUSED += [(m, 'period %r' % bad, dict(period=bad), _BAD, _PER % pwho) for bad in (0.0, np.nan, np.inf, -float(NX), NX - 1.0, NX - 2.0)]
_REFUSED += [(K12, 'nx == 1 with a period', dict(q=np.zeros((S, NY, 1)), period=1.0), _BAD, 'xc_contour_segments_periodic: nx >= 2'),
             (K11, 'a window of one row', dict(window=(1, 4)), _BAD, 'xc_local_contour_lengths: the window must be at least 2 x 2 nodes'),
             (K11, 'a window of one column', dict(window=(3, 1)), _BAD, 'xc_local_contour_lengths: the window must be at least 2 x 2 nodes'),
             (K11, 'a row stride of 0', dict(stride=(0, 1)), _BAD, 'xc_local_contour_lengths: strides must be >= 1'),
             (K11, 'a column stride of 0', dict(stride=(1, 0)), _BAD, 'xc_local_contour_lengths: strides must be >= 1'),
             (K11, 'wx > nx on a ring', dict(window=(3, NX + 1), period=PERIOD), _BAD,
              'xc_local_contour_lengths_periodic: the window must not be wider than the ring (wx <= nx)'),
             (K11, 'levels of a wrong shape', dict(levels=np.zeros((NWY, NWX + 1))), _BAD,
              'levels must be a scalar, (nwy, nwx) or (nslab, nwy, nwx)'),
             (K11, 'levels for other slabs', dict(levels=np.zeros((S + 1, NWY, NWX))), _BAD,
              'levels must be a scalar, (nwy, nwx) or (nslab, nwy, nwx)')]


@pytest.mark.parametrize('method,what,kw,code,text', _REFUSED, ids=['%s-%s' % r[:2] for r in _REFUSED])
def test_one_defect_one_error(ctx, q, method, what, kw, code, text):
    kw = dict(kw)
    q = kw.pop('q', q)
    if kw.pop('resident', False):
        _make_resident(ctx, q)
    with pytest.raises(nat.XContourHipError) as e:
        _call(ctx, method, q, **kw)
    assert e.value.code == code and str(e.value) == text
    assert ctx.lib.calls == [] and ctx._buffers == []               # refused before anything reached the library


def test_the_defect_free_calls_of_the_table_pass(ctx, q):
    for m in (K10, K11, K12, K13):
        for period in (None, PERIOD):
            _call(ctx, m, q, period=period)
    assert ctx._buffers == []
