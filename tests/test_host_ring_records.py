# -*- coding: utf-8 -*-
"""The host layer of the record kernels K14 - K23 (`contour_polylines` ... `contour_piece_tracks` of `_native.Context`), pinned without
a GPU, like test_host_batching.py does for K10 - K13: a Context over the stand-in library of standin_lib.py.  Pinned are the batches
and the per-slab byte estimate behind them, the order of the library calls with every argument (a device address as the bytes of
its allocation and the offset in it: the column layout of every record buffer), the allocations, every refusal text, and -- on
hand-built records served by scripted kernels -- the host arithmetic that turns the device's packed order into rows of the
first_edge-sorted tables."""
import numpy as np
import pytest

from standin_lib import _K12, _Lib

from xcontour_amd import _native as nat

S, NY, NX, N = 5, 6, 8, 4
CELLS = NY * NX
SLAB = CELLS * 8                        # bytes of one float64 slab
F64, F32 = nat.XC_F64, nat.XC_F32
BATCHES = [(0, 2), (2, 2), (4, 1)]      # (first slab, slabs) of the batches of S = 5
LV = np.linspace(-1, 1, N)
NSEG = 2                                # segments the scripted K12 finds in every range
W = np.ones((NY, NX))


def D(nbytes, off=0):
    return ('dev', nbytes, off)


@pytest.fixture
def ctx():
    c = nat.Context.__new__(nat.Context)
    c.lib, c.handle, c.device = _Lib(), None, 0
    c._buffers, c._resident, c._staged, c._ev_pool = [], {}, [], []
    c.max_batch_bytes = 8 << 30
    return c


@pytest.fixture
def q():
    return np.random.default_rng(7).standard_normal((S, NY, NX))


@pytest.fixture
def f():
    return np.random.default_rng(8).standard_normal((S, NY, NX))


def _take(ctx):
    """(calls, the arguments of every call as `_Lib.where` states them, mallocs) since the last _take"""
    lib = ctx.lib
    out = lib.calls, [tuple(lib.where(v) for v in a) for _, a in lib.args], lib.mallocs
    lib.calls, lib.args, lib.mallocs = [], [], []
    return out


def _k12(zero=()):
    """a scripted K12: NSEG segments in every range, none in the count-only calls numbered in `zero`; 1 from a count-only call that
    found segments, as the library's does"""
    seen = []

    def run(lib, a):
        if a[9]:
            return 0
        seen.append(1)
        n = 0 if len(seen) - 1 in zero else NSEG
        lib.poke(a[10], np.full(a[3] * a[7], n, dtype=np.uint64))
        return 1 if n else 0
    return run


def _rings(lib, a):
    """a scripted K18 - K21: two rings in every range, packed in descending first_edge, each holding one node; every node is labelled
    with packed position 0, which is row 1 of its range"""
    nr = a[1]
    lib.poke(a[16], np.full(nr, 2, dtype=np.uint64))
    lib.poke(a[17], np.tile(np.array([5, 3], dtype=np.int64), nr))
    lib.poke(a[19], np.ones(2 * nr, dtype=np.int32))
    if len(a) > 24:
        lib.poke(a[24], np.full(2 * nr, -1, dtype=np.int64))
        lib.poke(a[27], np.ones(2 * nr, dtype=np.int64))
    return 0


def _pairs(zero=()):
    """a scripted K22: one pair (0, 1) of 3 nodes in every range, none in the count-only calls numbered in `zero`"""
    seen = []

    def run(lib, a):
        nr = a[1]
        if a[11] == 0:
            seen.append(1)
            n = 0 if len(seen) - 1 in zero else 1
            lib.poke(a[12], np.full(nr, n, dtype=np.uint64))
            return 1 if n else 0
        lib.poke(a[13], np.zeros(nr, dtype=np.int32))
        lib.poke(a[14], np.ones(nr, dtype=np.int32))
        lib.poke(a[15], np.full(nr, 3, dtype=np.int64))
        return 0
    return run


def _install(ctx, zero=(1,), pairs_zero=()):
    ctx.lib.on = {_K12[0]: _k12(zero), 'xc_label_overlap_dev': _pairs(pairs_zero)}
    ctx.lib.on[_K12[1]] = ctx.lib.on[_K12[0]]
    for k in ('interiors', 'tree', 'labels', 'props'):
        ctx.lib.on['xc_contour_piece_%s_dev' % k] = _rings


def _batches_follow(ctx, per, call, count_calls=1):
    """`per` is the byte estimate of one slab: one byte less than two slabs' worth gives batches of one slab, two slabs' worth
    batches of 2, 2, 1 -- told by the slabs of K12's count-only calls (`count_calls` of them per batch)"""
    for cap, want in ((2 * per - 1, [1] * S), (2 * per, [2, 2, 1])):
        ctx.max_batch_bytes = cap
        _install(ctx, zero=())
        call()
        got = [a[3] for name, a in ctx.lib.args if name in _K12 and a[9] == 0]
        assert got == [n for n in want for _ in range(count_calls)]
        assert ctx._buffers == []
        _take(ctx)
    _install(ctx)


def _segments(n, periodic, total):
    """what K12's two calls of a batch of n slabs look like (shared levels), and the allocations before them"""
    head = (None, D(n * SLAB), F64, n, NY, NX, D(N * 8), N, 0)
    a = [head + (0, D(n * N * 8), None, None, None)]
    if total:
        a.append(head + (total, D(n * N * 8), D(total * 8), D(total * 8), D(total * 32)))
    return a


def _seq(seg, name, every_batch=False):
    out = []
    for b, (s0, n) in enumerate(BATCHES):
        out += [(seg, n)] + ([(seg, n)] if b != 1 else []) + ([(name, n * N)] if b != 1 or every_batch else [])
    return out


# ------------------------------------------------------------------ K14, K16, K17: one entry point on K12's records
@pytest.mark.parametrize('periodic', [False, True])
def test_contour_polylines(ctx, q, periodic):
    seg, K14 = _K12[periodic], 'xc_contour_polylines_dev'
    _batches_follow(ctx, SLAB, lambda: ctx.contour_polylines(q, LV, periodic=periodic))

    def polylines(lib, a):                                          # one polyline of both segments in every range
        lib.poke(a[9], np.ones(a[1], dtype=np.uint64))
        lib.poke(a[10], np.full(a[1], 2, dtype=np.int64))
        lib.poke(a[11], np.ones(a[1], dtype=np.int32))
        return 0
    ctx.lib.on[K14] = polylines
    res = ctx.contour_polylines(q, LV, periodic=periodic)
    calls, args, mallocs = _take(ctx)
    assert calls == _seq(seg, K14)
    want_m, want_a = [], []
    for b, (s0, n) in enumerate(BATCHES):
        t = 0 if b == 1 else NSEG * n * N
        want_m += [n * SLAB, N * 8, n * N * 8, n * N * 8] + ([t * 8, t * 8, t * 32, t * 8, t * 32, t * 20] if t else [])
        want_a += _segments(n, periodic, t)
        if t:
            want_a.append((None, n * N, D(n * N * 8), D(t * 8), D(t * 8), D(t * 32), NY, NX, t, D(n * N * 8),
                           D(t * 20), D(t * 20, 16 * t), D(t * 20, 8 * t), D(t * 32), D(t * 8), None))
    assert mallocs == want_m and args == want_a
    cnt, efw, ptw, poly_off, closed, rpo = res
    assert cnt.shape == (S, N) and cnt.dtype == np.uint64 and cnt[:, 0].tolist() == [2, 2, 0, 0, 2]
    assert efw.shape == (24,) and efw.dtype == np.int64 and ptw.shape == (24, 4) and ptw.dtype == np.float64
    assert poly_off.dtype == np.int64 and poly_off.tolist() == list(range(0, 25, 2))
    assert closed.dtype == np.bool_ and closed.tolist() == [True] * 12
    assert rpo.dtype == np.int64 and rpo.tolist() == list(range(9)) + [8] * 8 + list(range(9, 13))
    assert ctx._buffers == []
    ctx.lib.on, ctx.max_batch_bytes = {}, 8 << 30                   # nothing anywhere: K14 is never run
    res = ctx.contour_polylines(q, LV, periodic=periodic)
    calls, args, mallocs = _take(ctx)
    assert calls == [(seg, S)] and mallocs == [S * SLAB, N * 8, S * N * 8, S * N * 8]
    assert [r.shape for r in res] == [(S, N), (0,), (0, 4), (1,), (0,), (S * N + 1,)] and not res[5].any()
    assert [r.dtype for r in res] == [np.uint64, np.int64, np.float64, np.int64, np.bool_, np.int64]
    assert ctx._buffers == []


@pytest.mark.parametrize('periodic,select,sel', [(False, 'all', 0), (True, 'main', 2), (True, 1, 1)])
def test_contour_overturning(ctx, q, periodic, select, sel):
    seg, K16 = _K12[periodic], 'xc_contour_overturning_dev'
    _batches_follow(ctx, SLAB + N * NX * 20, lambda: ctx.contour_overturning(q, LV, periodic=periodic, select=select))
    ctx.lib.on[K16] = lambda lib, a: (lib.poke(a[10], np.full(a[1] * NX, 3, dtype=np.int32)), 0)[1]
    res = ctx.contour_overturning(q, LV, periodic=periodic, select=select)
    calls, args, mallocs = _take(ctx)
    assert calls == _seq(seg, K16)
    want_m, want_a = [], []
    for b, (s0, n) in enumerate(BATCHES):
        t = 0 if b == 1 else NSEG * n * N
        outs = [n * N * k for k in (NX * 4, NX * 8, NX * 8, 4, 8, 8, 4)]
        want_m += [n * SLAB, N * 8, n * N * 8] + outs + ([t * 8, t * 8, t * 32] if t else [])
        want_a += _segments(n, periodic, t)
        if t:
            want_a.append((None, n * N, D(n * N * 8), D(t * 8), D(t * 8), D(t * 32), NY, NX, int(periodic), sel) + tuple(D(k) for k in outs))
    assert mallocs == want_m and args == want_a
    assert [r.shape for r in res] == [(S, N, NX)] * 3 + [(S, N)] * 4
    assert [r.dtype for r in res] == [np.int32, np.float64, np.float64, np.int32, np.int64, np.int64, np.int32]
    assert (res[0][[0, 1, 4]] == 3).all() and not res[0][[2, 3]].any()
    # the batch without segments: no crossing, NaN rows, nothing selected, no main ring
    assert np.isnan(res[1][2:4]).all() and np.isnan(res[2][2:4]).all() and (res[4][2:4] == -1).all()
    assert not res[3][2:4].any() and not res[5][2:4].any() and not res[6][2:4].any()
    assert ctx._buffers == []


@pytest.mark.parametrize('mask', [False, True])
@pytest.mark.parametrize('w_per_slab,has_f', [(False, False), (False, True), (True, True)])
def test_contour_interior(ctx, q, f, w_per_slab, has_f, mask):
    seg, K17 = _K12[1], 'xc_contour_interior_dev'
    w = np.ones((S, NY, NX)) if w_per_slab else W
    g = f.astype(np.float32) if has_f else None

    def call():
        return ctx.contour_interior(q, LV, w=w, f=g, periodic=True, select='circumpolar', flip=True, return_mask=mask)
    _batches_follow(ctx, CELLS * (8 + (8 if w_per_slab else 0) + (4 if has_f else 0) + (N if mask else 0)), call)
    res = call()
    calls, args, mallocs = _take(ctx)
    assert calls == _seq(seg, K17, every_batch=True)                # K17 runs without segments too: everything is outside
    want_m, want_a = [], []
    for b, (s0, n) in enumerate(BATCHES):
        t = 0 if b == 1 else NSEG * n * N
        ins = [n * SLAB if w_per_slab else SLAB] + ([n * CELLS * 4] if has_f else [])
        outs = [n * N * 8] * (3 if has_f else 2) + ([n * N * CELLS] if mask else [])
        want_m += [n * SLAB, N * 8] + ins + [n * N * 8] + outs + ([t * 8, t * 8, t * 32] if t else [])
        want_a += _segments(n, True, t)
        recs = (D(t * 8), D(t * 8), D(t * 32)) if t else (None, None, None)
        want_a.append((None, n * N, D(n * N * 8)) + recs + (NY, NX, 1, 1, 1, N, D(ins[0]), int(w_per_slab), D(ins[1]) if has_f else None,
                                                            F32 if has_f else 0, D(n * N * 8), D(n * N * 8), D(n * N * 8) if has_f else None,
                                                            D(n * N * CELLS) if mask else None))
    assert mallocs == want_m and args == want_a
    assert len(res) == (4 if mask else 3)
    assert res[0].shape == res[1].shape == (S, N) and res[0].dtype == np.int64 and res[1].dtype == np.float64
    assert (res[2] is None) if not has_f else (res[2].shape == (S, N) and res[2].dtype == np.float64)
    assert not mask or (res[3].shape == (S, N, NY, NX) and res[3].dtype == np.bool_)
    assert ctx._buffers == []


# ------------------------------------------------------------------ K18 - K21: the ring records
def _ring_head(n, t, B, has_f, tree):
    """the arguments the four ring entry points share for a batch of n slabs: w one plane, f float64 per slab; B the bytes of one
    record: the 8-byte columns, then the 4-byte ones"""
    c8 = 9 if tree else 5
    R = lambda k: D(t * B, k * 8 * t)                               # noqa: E731
    R4 = lambda k: D(t * B, (8 * c8 + 4 * k) * t)                   # noqa: E731
    a = (None, n * N, D(n * N * 8), D(t * 8), D(t * 8), D(t * 32), NY, NX, 1, 1, N, D(SLAB), 0, D(n * SLAB) if has_f else None,
         F64 if has_f else 0, t, D(n * N * 8), R(0), R(1), R4(0), R4(1), R(2), R(3), R(4) if has_f else None)
    if tree:
        a += (R(5), R4(2), R4(3), R(6), R(7), R(8) if has_f else None)
    return a


@pytest.mark.parametrize('has_f', [False, True])
@pytest.mark.parametrize('method', ['interiors', 'tree', 'labels'])
def test_ring_records(ctx, q, f, method, has_f):
    seg, name = _K12[1], 'xc_contour_piece_%s_dev' % method
    tree, g = method != 'interiors', f if has_f else None
    B = 88 if tree else 48

    def call():
        return getattr(ctx, 'contour_piece_' + method)(q, LV, w=W, f=g, periodic=True, flip=True)
    _batches_follow(ctx, CELLS * (8 + (8 if has_f else 0) + (4 * N if method == 'labels' else 0)), call)
    res = call()
    calls, args, mallocs = _take(ctx)
    assert calls == _seq(seg, name)
    want_m, want_a = [], []
    for b, (s0, n) in enumerate(BATCHES):
        t = 0 if b == 1 else NSEG * n * N
        want_m += [n * SLAB, N * 8, SLAB] + ([n * SLAB] if has_f else []) + [n * N * 8, n * N * 8]
        want_m += ([n * N * CELLS * 4] if method == 'labels' else []) + ([t * 8, t * 8, t * 32, t * B] if t else [])
        want_a += _segments(n, True, t)
        if t:
            want_a.append(_ring_head(n, t, B, has_f, tree) + ((D(n * N * CELLS * 4),) if method == 'labels' else ()))
    # the label map of a batch may be allocated before or after the batch's other buffers: the allocations as a set
    assert (sorted(mallocs) == sorted(want_m)) if method == 'labels' else (mallocs == want_m)
    assert args == want_a
    pc, tab = res[:2]
    assert len(res) == (3 if method == 'labels' else 2)
    assert pc.shape == (S, N) and pc.dtype == np.uint64 and pc[:, 0].tolist() == [2, 2, 0, 0, 2]
    assert tab.dtype == (nat.Context.PIECE_TREE_DTYPE if tree else nat.Context.PIECE_INTERIOR_DTYPE)
    assert tab['first_edge'].tolist() == [3, 5] * 12 and tab['closed'].all()
    assert np.isnan(tab['sum_wf']).all() if not has_f else not tab['sum_wf'].any()
    if tree:
        assert (tab['parent'] == -1).all() and (tab['n_net'] == 1).all()
        assert np.isnan(tab['net_wf']).all() if not has_f else not tab['net_wf'].any()
    if method == 'labels':
        lab = res[2]
        assert lab.shape == (S, N, NY, NX) and lab.dtype == np.int32
        assert (lab[[0, 1, 4]] == 1).all() and (lab[[2, 3]] == -1).all()          # packed position 0 is row 1; no ring without segments
    assert ctx._buffers == []
    ctx.lib.on, ctx.max_batch_bytes = {}, 8 << 30                   # nothing anywhere
    res = call()
    calls, args, mallocs = _take(ctx)
    assert calls == [(seg, S)] and ctx._buffers == []
    assert res[0].shape == (S, N) and not res[0].any() and res[1].shape == (0,) and res[1].dtype == tab.dtype
    assert method != 'labels' or (res[2].shape == (S, N, NY, NX) and res[2].dtype == np.int32 and (res[2] == -1).all())


@pytest.mark.parametrize('has_x', [False, True])
def test_ring_props(ctx, q, f, has_x):
    seg, K21 = _K12[1], 'xc_contour_piece_props_dev'
    fields = [np.ones((NY, NX), dtype=np.float32), f]
    x = q if has_x else None

    def call(fields=fields):
        return ctx.contour_piece_props(q, LV, w=W, fields=fields, x=x, periodic=True, flip=True)
    _batches_follow(ctx, CELLS * (8 + 8 + (8 if has_x else 0)), call)

    def props(lib, a):
        _rings(lib, a)
        t = a[15]
        net = np.zeros((2, t))
        net[0, :2 * a[1]], net[1, :2 * a[1]] = np.tile([10.0, 20.0], a[1]), np.tile([30.0, 40.0], a[1])
        lib.poke(a[36], net)
        lib.poke(a[37], -net)
        if a[38]:
            lib.poke(a[38], np.tile([1.5, 2.5], a[1]))
            lib.poke(a[41], np.tile(np.array([7, 9], dtype=np.int64), a[1]))
        return 0
    ctx.lib.on[K21] = props
    pc, tab, pr = call()
    calls, args, mallocs = _take(ctx)
    assert calls == _seq(seg, K21)
    B = 88 + 8 * (2 * 2 + 4)
    want_m, want_a = [], []
    for b, (s0, n) in enumerate(BATCHES):
        t = 0 if b == 1 else NSEG * n * N
        want_m += [n * SLAB, N * 8, SLAB, CELLS * 4, n * SLAB] + ([n * SLAB] if has_x else []) + [n * N * 8, n * N * 8]
        want_m += [t * 8, t * 8, t * 32, t * B] if t else []
        want_a += _segments(n, True, t)
        if t:
            P = lambda k: D(t * B, (88 + 8 * k) * t)                # noqa: E731
            want_a.append(_ring_head(n, t, B, False, True) + (2, 'host', 'host', 'host', D(n * SLAB) if has_x else None,
                                                              F64 if has_x else 0, P(0), P(2))
                          + (tuple(P(k) for k in (4, 5, 6, 7)) if has_x else (None,) * 4))
    assert mallocs == want_m and args == want_a
    assert tab.dtype == nat.Context.PIECE_TREE_DTYPE and tab['first_edge'].tolist() == [3, 5] * 12
    assert list(pr) == ['net', 'gross', 'x_min', 'x_max', 'at_min', 'at_max']
    assert pr['net'].shape == (24, 2) and pr['net'].flags.c_contiguous
    assert pr['net'].tolist() == [[20.0, 40.0], [10.0, 30.0]] * 12 and (pr['gross'] == -pr['net']).all()
    if has_x:
        assert pr['x_min'].tolist() == [2.5, 1.5] * 12 and pr['at_max'].tolist() == [9, 7] * 12 and pr['at_max'].dtype == np.int64
        assert not pr['x_max'].any() and pr['x_max'].shape == (24,)
    else:
        assert pr['x_min'] is pr['x_max'] is pr['at_min'] is pr['at_max'] is None
    assert ctx._buffers == []
    ctx.lib.on, ctx.max_batch_bytes = {}, 8 << 30                   # nothing anywhere; and no fields
    pc, tab, pr = call(fields=())
    calls, args, mallocs = _take(ctx)
    assert calls == [(seg, S)] and ctx._buffers == []
    assert not pc.any() and tab.shape == (0,) and pr['net'].shape == pr['gross'].shape == (0, 0)
    assert (pr['x_min'] is None) if not has_x else (pr['x_min'].shape == (0,) and pr['at_min'].dtype == np.int64)


# ------------------------------------------------------------------ K22
def _overlap_calls(nr, T, pa, pb, pw, pf, f_code):
    head = (None, nr, NY, NX, N, pa, pb, pw, 0, pf, f_code)
    out = [head + (0, D(nr * 8), None, None, None, None, None)]
    if T:
        out.append(head + (T, D(nr * 8), D(T * 32), D(T * 32, 4 * T), D(T * 32, 8 * T), D(T * 32, 16 * T),
                           D(T * 32, 24 * T) if pf else None))
    return out


@pytest.mark.parametrize('has_f', [False, True])
def test_label_overlap(ctx, f, has_f):
    K22 = 'xc_label_overlap_dev'
    la = np.zeros((S, N, NY, NX), dtype=np.int32)
    g = f if has_f else None
    for cap, want in ((2 * CELLS * (8 * N + (8 if has_f else 0)) - 1, [N] * S), (2 * CELLS * (8 * N + (8 if has_f else 0)), [2 * N, 2 * N, N])):
        ctx.max_batch_bytes = cap
        ctx.lib.on = {K22: _pairs(zero=(1,))}
        pc, rows = ctx.label_overlap(la, la + 1, w=W, f=g)
        calls, args, mallocs = _take(ctx)
        assert [n for _, n in calls] == [n for b, n in enumerate(want) for _ in range(1 if b == 1 else 2)]
    want_m, want_a = [], []
    for b, (s0, n) in enumerate(BATCHES):
        T = 0 if b == 1 else n * N
        m = n * N * CELLS * 4
        want_m += [m, m, SLAB] + ([n * SLAB] if has_f else []) + [n * N * 8] + ([T * 32] if T else [])
        want_a += _overlap_calls(n * N, T, D(m), D(m), D(SLAB), D(n * SLAB) if has_f else None, F64 if has_f else 0)
    assert mallocs == want_m and args == want_a
    assert pc.shape == (S, N) and pc.dtype == np.uint64 and pc[:, 0].tolist() == [1, 1, 0, 0, 1]
    assert rows.dtype == nat.Context.OVERLAP_DTYPE and rows.shape == (12,)
    assert rows['a'].tolist() == [0] * 12 and rows['b'].tolist() == [1] * 12 and rows['n'].tolist() == [3] * 12
    assert np.isnan(rows['sum_wf']).all() if not has_f else not rows['sum_wf'].any()
    assert ctx._buffers == []
    ctx.max_batch_bytes = 8 << 30                                   # (nrange, ny, nx) maps: every range its own slab
    ctx.lib.on = {K22: _pairs()}
    pc, rows = ctx.label_overlap(la[0], la[0])
    calls, args, mallocs = _take(ctx)
    assert calls == [(K22, N), (K22, N)] and args[0][1:5] == (N, NY, NX, 1) and pc.shape == (N,) and rows.shape == (N,)


@pytest.mark.parametrize('has_f', [False, True])
def test_contour_piece_overlap(ctx, q, f, has_f):
    seg, K20, K22 = _K12[1], 'xc_contour_piece_labels_dev', 'xc_label_overlap_dev'
    g, qb = (f if has_f else None), q[::-1].astype(np.float32)

    def call():
        return ctx.contour_piece_overlap(q, qb, LV, contours_b=LV + 0.5, w=W, f=g, periodic=True, flip=True)
    _batches_follow(ctx, CELLS * (8 + 4 + 8 * N + (8 if has_f else 0)), call, count_calls=2)
    _install(ctx, zero=(2, 3), pairs_zero=(1,))                     # the second batch: no segments in either field, no pairs
    res = call()
    k22 = [a for name, a in ctx.lib.args if name == K22]
    calls, args, mallocs = _take(ctx)
    # ... and K22 meets there two maps that say "no ring" everywhere
    assert all((np.frombuffer(ctx.lib.mem[p], dtype=np.int32) == -1).all() and len(ctx.lib.mem[p]) == 2 * N * CELLS * 4 for p in k22[2][5:7])
    want_c, want_m, want_a = [], [], []
    for b, (s0, n) in enumerate(BATCHES):
        t = 0 if b == 1 else NSEG * n * N
        T = 0 if b == 1 else n * N
        m = n * N * CELLS * 4
        want_m += [m, m]
        for slab in (SLAB, SLAB // 2):
            want_c += [(seg, n)] + ([(seg, n), (K20, n * N)] if t else [])
            want_m += [n * slab, N * 8, SLAB] + ([n * SLAB] if has_f else []) + [n * N * 8, n * N * 8] + ([t * 8, t * 8, t * 32, t * 88] if t else [])
            k12 = _segments(n, True, t)
            if slab != SLAB:
                k12 = [a[:1] + (D(n * slab), F32) + a[3:] for a in k12]
            want_a += k12 + ([_ring_head(n, t, 88, has_f, True) + (D(m),)] if t else [])
        want_c += [(K22, n * N)] * (2 if T else 1)
        want_m += [SLAB] + ([n * SLAB] if has_f else []) + [n * N * 8] + ([T * 32] if T else [])
        want_a += _overlap_calls(n * N, T, D(m), D(m), D(SLAB), D(n * SLAB) if has_f else None, F64 if has_f else 0)
    assert calls == want_c and mallocs == want_m and args == want_a
    pc_a, tab_a, pc_b, tab_b, pairs, rows = res
    for pc, tab in ((pc_a, tab_a), (pc_b, tab_b)):
        assert pc.shape == (S, N) and pc[:, 0].tolist() == [2, 2, 0, 0, 2] and tab.dtype == nat.Context.PIECE_TREE_DTYPE
        assert tab['first_edge'].tolist() == [3, 5] * 12
    assert pairs.shape == (S, N) and pairs.dtype == np.uint64 and pairs[:, 0].tolist() == [1, 1, 0, 0, 1]
    # the device's pair (0, 1) are packed positions: -> rows (1, 0) of the sorted tables
    assert rows.dtype == nat.Context.OVERLAP_DTYPE and rows['a'].tolist() == [1] * 12 and rows['b'].tolist() == [0] * 12
    assert ctx._buffers == []


# ------------------------------------------------------------------ K23
RING = 'xc_ring_tracks_dev'


def _tracks_kernel(nt, stride=None):
    """a scripted K23 of nt tracks: every column its own values -- or, with `stride`, track k beginning with ring k * stride at
    step 0 and nothing else"""
    def run(lib, a):
        nring = a[1]
        if a[14] == 0:
            lib.poke(a[15], np.array([nt], dtype=np.uint64))
            return 1 if nt else 0
        if stride:
            lib.poke(a[10], np.arange(nring, dtype=np.int64) // stride)
            lib.poke(a[13], np.ones(a[2], dtype=np.uint8))
            lib.poke(a[16], np.arange(nt, dtype=np.int64) * stride)
            return 0
        lib.poke(a[9], np.arange(nring, dtype=np.int64))            # root
        lib.poke(a[10], np.arange(nring, dtype=np.int64) % nt)      # track
        lib.poke(a[11], np.full(nring, 1, dtype=np.int32))
        lib.poke(a[12], np.full(nring, 2, dtype=np.int32))
        lib.poke(a[13], np.ones(a[2], dtype=np.uint8))
        for p, t, v in zip(a[16:], (np.int64, np.int32, np.int32, np.int64, np.int64, np.int64), (0, 1, 2, 3, 4, 5)):
            lib.poke(p, np.arange(nt).astype(t) * 10 + v)
        return 0
    return run


def _ring_track_calls(nring, nlink, nt, mo, sized=True):
    head = (None, nring, nlink, D(nring * 4), D(nring * 8)) + ((D(nlink * 8),) * 3 if nlink else (None,) * 3) + (mo,)
    R, T = 24 * nring, 40 * nt
    return [head + (None,) * 5 + (0, D(8)) + (None,) * 6,
            head + (D(R), D(R, 8 * nring), D(R, 16 * nring), D(R, 20 * nring), D(max(nlink, 1)), nt, D(8),
                    D(T), D(T, 32 * nt), D(T, 36 * nt), D(T, 8 * nt), D(T, 16 * nt), D(T, 24 * nt))]


@pytest.mark.parametrize('nlink', [0, 5])
def test_ring_tracks(ctx, nlink):
    ctx.lib.on = {RING: _tracks_kernel(3)}
    link = np.arange(nlink)
    out = ctx.ring_tracks(np.arange(7) // 2, np.ones(7), link, link + 1, link + 2, min_overlap=0.25)
    calls, args, mallocs = _take(ctx)
    assert calls == [(RING, 7), (RING, 7)]                          # a count-only call, then the sized one
    assert mallocs == [7 * 4, 7 * 8] + ([nlink * 8] * 3 if nlink else []) + [8, 7 * 24, max(nlink, 1), 3 * 40]
    assert args == _ring_track_calls(7, nlink, 3, 0.25)
    assert list(out) == ['root', 'track', 'nprev', 'nnext', 'link_ok', 'tracks']
    assert out['root'].tolist() == list(range(7)) and out['track'].tolist() == [0, 1, 2, 0, 1, 2, 0]
    assert out['nprev'].tolist() == [1] * 7 and out['nnext'].tolist() == [2] * 7 and out['nprev'].dtype == out['nnext'].dtype == np.int32
    assert out['link_ok'].dtype == np.bool_ and out['link_ok'].tolist() == [True] * nlink
    tr = out['tracks']
    assert tr.dtype == nat.Context.TRACK_DTYPE
    assert [tr[k].tolist() for k in tr.dtype.names] == [[v, 10 + v, 20 + v] for v in range(6)]
    assert ctx._buffers == []
    out = ctx.ring_tracks(np.zeros(0), None, link[:0], link[:0], link[:0])            # no rings: the library is not asked
    assert _take(ctx) == ([], [], []) and out['tracks'].shape == (0,) and out['tracks'].dtype == nat.Context.TRACK_DTYPE
    assert [out[k].dtype for k in ('root', 'track', 'nprev', 'nnext', 'link_ok')] == [np.int64, np.int64, np.int32, np.int32, np.bool_]


@pytest.mark.parametrize('w_per_slab', [False, True])
def test_contour_piece_tracks(ctx, q, f, w_per_slab):
    seg, K20, K22 = _K12[1], 'xc_contour_piece_labels_dev', 'xc_label_overlap_dev'
    w = np.ones((S, NY, NX)) if w_per_slab else W
    ws = (lambda n: n * SLAB) if w_per_slab else (lambda n: SLAB)

    def call():
        return ctx.contour_piece_tracks(q, LV, w=w, f=f, periodic=True, flip=True, min_overlap=0.5)
    per = CELLS * (8 + 4 * N + (8 if w_per_slab else 0) + 8)
    ctx.max_batch_bytes = 2 * per - 1
    _install(ctx, zero=())
    ctx.lib.on[RING] = _tracks_kernel(N, stride=2 * S)
    call()
    assert [n for name, n in _take(ctx)[0] if name == K20] == [N] * S
    ctx.max_batch_bytes = 2 * per
    _install(ctx, zero=())
    ctx.lib.on[RING] = _tracks_kernel(N, stride=2 * S)
    res = call()
    calls, args, mallocs = _take(ctx)
    slot = N * CELLS * 4
    want_c, want_m, want_a = [], [3 * slot], []
    for b, (s0, n) in enumerate(BATCHES):
        t = NSEG * n * N
        npair = n - 1 if b == 0 else n                              # the first batch has no step before it
        T = npair * N
        # one label call per batch, on all its steps, into slots 1 .. n of the map buffer; then ONE overlap pair of calls per batch,
        # slots [first, first + npair) against the slots one on
        want_c += [(seg, n), (seg, n), (K20, n * N), (K22, T), (K22, T)]
        want_m += [n * SLAB, N * 8, ws(n), n * SLAB, n * N * 8, n * N * 8, t * 8, t * 8, t * 32, t * 88]
        want_m += [ws(npair), T * 8, T * 32]
        head = _ring_head(n, t, 88, True, True)
        want_a += _segments(n, True, t) + [head[:11] + (D(ws(n)), int(w_per_slab)) + head[13:] + (D(3 * slot, slot),)]
        first = 1 if b == 0 else 0
        ov = _overlap_calls(T, T, D(3 * slot, first * slot), D(3 * slot, (first + 1) * slot), D(ws(npair)), None, 0)
        want_a += [a[:8] + (int(w_per_slab),) + a[9:] for a in ov]
    nring, nlink = 2 * S * N, (S - 1) * N
    want_c += [(RING, nring), (RING, nring)]
    want_m += [nring * 4, nring * 8, nlink * 8, nlink * 8, nlink * 8, 8, nring * 24, nlink, N * 40]
    want_a += _ring_track_calls(nring, nlink, N, 0.5)
    assert calls == want_c and mallocs == want_m and args == want_a
    pc, tab, ring, lc, links, tc, tracks = res
    assert pc.shape == (S, N) and (pc == 2).all() and tab.dtype == nat.Context.PIECE_TREE_DTYPE and tab.shape == (2 * S * N,)
    assert ring.dtype == nat.Context.RING_TRACK_DTYPE and ring.shape == tab.shape
    assert lc.shape == (S - 1, N) and lc.dtype == np.uint64 and (lc == 1).all()
    assert links.dtype == nat.Context.TRACK_LINK_DTYPE and links.shape == (nlink,)
    assert links['step'].tolist() == [t for t in range(S - 1) for _ in range(N)]
    # packed positions (0, 1) -> rows (1, 0), across the batch boundaries too (the earlier step's rows are the batch before's)
    assert links['a'].tolist() == [1] * nlink and links['b'].tolist() == [0] * nlink and links['linked'].all()
    assert tc.shape == (N,) and tc.dtype == np.uint64 and tracks.dtype == nat.Context.PIECE_TRACK_DTYPE and tracks.shape == (N,)
    assert ctx._buffers == []


def test_what_k23_is_given_and_what_becomes_of_its_answer(ctx, q):
    """three steps, one level, batches of 2 and 1 steps; rings per step 2, 1, 2 with hand-built records"""
    fe = {0: [9, 4], 1: [6], 2: [2, 8]}                             # first_edge as packed: step 0 and 2 sort to [1, 0] / [0, 1]
    net = {0: [30, 40], 1: [50], 2: [60, 70]}
    pairs = {0: [(0, 0, 5), (1, 0, 6)], 1: [(0, 1, 7), (0, -1, 2)]}  # (a, b, n) per pair of steps, packed positions
    step_of = []

    def k12(lib, a):
        if a[9] == 0:
            lib.poke(a[10], np.full(a[3], 2, dtype=np.uint64))
            return 1
        return 0

    def k20(lib, a):
        steps = [len(step_of) + j for j in range(a[1])]
        step_of.extend(steps)
        lib.poke(a[16], np.array([len(fe[s]) for s in steps], dtype=np.uint64))
        lib.poke(a[17], np.array(sum((fe[s] for s in steps), []), dtype=np.int64))
        lib.poke(a[19], np.ones(5, dtype=np.int32))
        lib.poke(a[24], np.full(5, -1, dtype=np.int64))
        lib.poke(a[27], np.array(sum((net[s] for s in steps), []), dtype=np.int64))
        return 0
    seen = []

    def k22(lib, a):
        if a[11] == 0:
            seen.append(len(seen))
            lib.poke(a[12], np.array([len(pairs[seen[-1]])], dtype=np.uint64))
            return 1
        rows = pairs[seen[-1]]
        for p, j, t in ((a[13], 0, np.int32), (a[14], 1, np.int32), (a[15], 2, np.int64)):
            lib.poke(p, np.array([r[j] for r in rows], dtype=t))
        return 0
    def k23(lib, a):
        if a[14] == 0:
            lib.poke(a[15], np.array([2], dtype=np.uint64))
            return 1
        lib.poke(a[10], np.array([0, 0, 0, 0, 1], dtype=np.int64))
        lib.poke(a[13], np.array([1, 1, 1, 0], dtype=np.uint8))
        lib.poke(a[16], np.array([0, 4], dtype=np.int64))           # first_ring
        lib.poke(a[17], np.array([0, 2], dtype=np.int32))           # first_step
        return 0
    ctx.lib.on = {_K12[0]: k12, 'xc_contour_piece_labels_dev': k20, 'xc_label_overlap_dev': k22, RING: k23}
    ctx.max_batch_bytes = 2 * CELLS * (8 + 4)
    pc, tab, ring, lc, links, tc, tracks = ctx.contour_piece_tracks(q[:3], LV[:1])
    assert [n for name, n in ctx.lib.calls if name.startswith('xc_contour_piece')] == [2, 1]
    assert pc.ravel().tolist() == [2, 1, 2] and tab['first_edge'].tolist() == [4, 9, 6, 2, 8] and tab['n_net'].tolist() == [40, 30, 50, 60, 70]
    assert lc.ravel().tolist() == [2, 2]
    # a / b: packed position -> row of the step's sorted table; each range sorted by (a, b)
    assert [tuple(r) for r in links[['step', 'a', 'b', 'n']].tolist()] == [(0, 0, 0, 6), (0, 1, 0, 5), (1, 0, -1, 2), (1, 0, 1, 7)]
    # what K23 was given: the rings level-major in (step, row) order, the links as ring indices
    given = [a for name, a in ctx.lib.args if name == RING][0]
    ring_step, ring_size, la, lb, ln = (np.frombuffer(ctx.lib.mem[p], dtype=t)
                                        for p, t in zip(given[3:8], (np.int32, np.int64, np.int64, np.int64, np.int64)))
    assert ring_step.tolist() == [0, 0, 1, 2, 2] and ring_size.tolist() == [40, 30, 50, 60, 70]
    assert la.tolist() == [0, 1, 2, 2] and lb.tolist() == [2, 2, -1, 4] and ln.tolist() == [6, 5, 2, 7]
    assert links['linked'].tolist() == [True, True, True, False]
    assert ring['track'].tolist() == [0, 0, 0, 0, 1] and tc.tolist() == [2]
    assert tracks['first_step'].tolist() == [0, 2] and tracks['first_row'].tolist() == [0, 1]
    assert ctx._buffers == []


# ------------------------------------------------------------------ packed order -> rows of the sorted tables, on hand-built records
# two ranges (one slab, two levels) of three and two pieces, as the device packs them; the last piece is open
FE = [40, 10, 30, 7, 5]                                             # first_edge: range 0 sorts to packed 1, 2, 0; range 1 to packed 4, 3
PARENT = [1, -1, 0, 4, -1]                                          # an index into the packed rows of the call
SORTED = [1, 2, 0, 4, 3]                                            # the packed position of every row of the sorted table
ROW = {0: 2, 1: 0, 2: 1, 3: 1, 4: 0}                                # the row in its range's sorted table of every packed position
LABELS = np.array([[[-1, 0, 1, 2], [2, 2, 1, 0]], [[0, 1, -1, -1], [1, 1, 0, 0]]], dtype=np.int32)      # positions inside the range


def _hand_built(lib, a):
    lib.poke(a[16], np.array([3, 2], dtype=np.uint64))
    lib.poke(a[17], np.array(FE, dtype=np.int64))
    lib.poke(a[18], np.arange(5, dtype=np.int64) + 100)             # nseg: tells the pieces apart
    lib.poke(a[19], np.array([1, 1, 1, 1, 0], dtype=np.int32))
    lib.poke(a[22], np.arange(5) * 1.5)
    if len(a) > 24:
        lib.poke(a[24], np.array(PARENT, dtype=np.int64))
        lib.poke(a[25], np.array([1, 0, 2, 1, 0], dtype=np.int32))
    if len(a) == 31:
        lib.poke(a[30], LABELS)
    return 0


def _hand_k12(lib, a):
    if a[9] == 0:
        lib.poke(a[10], np.array([4, 3], dtype=np.uint64))
        return 1
    return 0


@pytest.mark.parametrize('method', ['interiors', 'tree', 'labels', 'props'])
def test_sorted_table_parent_rows_and_label_rows(ctx, method):
    q1 = np.zeros((1, 2, 4))
    ctx.lib.on = {_K12[0]: _hand_k12, 'xc_contour_piece_%s_dev' % method: _hand_built}
    res = getattr(ctx, 'contour_piece_' + method)(q1, LV[:2])
    pc, tab = res[:2]
    assert pc.tolist() == [[3, 2]]
    assert tab['first_edge'].tolist() == [10, 30, 40, 5, 7]
    assert tab['nseg'].tolist() == [100 + p for p in SORTED] and tab['sum_w'].tolist() == [1.5 * p for p in SORTED]
    assert tab['closed'].tolist() == [True, True, True, False, True] and tab['closed'].dtype == np.bool_
    if method != 'interiors':
        # packed index of the parent -> its row in the piece's own range
        assert tab['parent'].tolist() == [-1, 2, 0, -1, 0] and tab['depth'].tolist() == [0, 2, 1, 0, 1]
    if method == 'labels':
        want = [[[-1, 2, 0, 1], [1, 1, 0, 2]], [[1, 0, -1, -1], [0, 0, 1, 1]]]
        assert res[2].shape == (1, 2, 2, 4) and res[2].dtype == np.int32 and res[2][0].tolist() == want
    assert ctx._buffers == []


def test_overlap_rows_name_rows_of_the_sorted_tables(ctx):
    q1 = np.zeros((1, 2, 4))
    fe_b = [3, 8, 1, 2, 9]                                          # the other field: range 0 sorts to packed 2, 0, 1; range 1 to 3, 4
    nth = []

    def labels(lib, a):
        _hand_built(lib, a)
        nth.append(1)
        if len(nth) == 2:
            lib.poke(a[17], np.array(fe_b, dtype=np.int64))
        return 0
    # (a, b) as packed positions inside the range: range 0 three pairs, range 1 two
    pa, pb = [2, 0, 1, 1, -1], [1, -1, 2, 0, 1]

    def k22(lib, a):
        if a[11] == 0:
            lib.poke(a[12], np.array([3, 2], dtype=np.uint64))
            return 1
        lib.poke(a[13], np.array(pa, dtype=np.int32))
        lib.poke(a[14], np.array(pb, dtype=np.int32))
        lib.poke(a[15], np.arange(5, dtype=np.int64) + 1)
        return 0
    ctx.lib.on = {_K12[0]: _hand_k12, 'xc_contour_piece_labels_dev': labels, 'xc_label_overlap_dev': k22}
    pc_a, tab_a, pc_b, tab_b, pairs, rows = ctx.contour_piece_overlap(q1, q1, LV[:2])
    assert tab_a['first_edge'].tolist() == [10, 30, 40, 5, 7] and tab_b['first_edge'].tolist() == [1, 3, 8, 2, 9]
    assert tab_a['parent'].tolist() == [-1, 2, 0, -1, 0]
    assert pairs.tolist() == [[3, 2]]
    # a: rows of table_a (2 -> 1, 0 -> 2, 1 -> 0 | 1 -> 0, -1); b: rows of table_b (1 -> 2, -1, 2 -> 0 | 0 -> 0, 1 -> 1); sorted by (a, b)
    assert [tuple(r) for r in rows[['a', 'b', 'n']].tolist()] == [(0, 0, 3), (1, 2, 1), (2, -1, 2), (-1, 1, 5), (0, 0, 4)]
    assert np.isnan(rows['sum_wf']).all()
    assert ctx._buffers == []


# ------------------------------------------------------------------ what the methods refuse, and in which words
class _Huge(object):
    """a stack of one 32768 x 32768 plane that is never read: 2 ny nx = 2^31"""
    _xc_lazy_stack, shape, dtype = True, (1, 1 << 15, 1 << 15), np.dtype(np.float32)


def _call(ctx, method, q, contours=LV, **kw):
    if method in ('contour_piece_overlap',):
        qb = kw.pop('qb', q)
        return ctx.contour_piece_overlap(q, qb, contours, **kw)
    if method == 'label_overlap':
        return ctx.label_overlap(kw.pop('a', np.zeros((S, N, NY, NX), dtype=np.int32)), kw.pop('b', np.zeros((S, N, NY, NX), dtype=np.int32)), **kw)
    if method == 'ring_tracks':
        args = dict(ring_step=np.zeros(4), ring_size=np.ones(4), link_a=np.zeros(3), link_b=np.zeros(3), link_n=np.ones(3))
        args.update(kw)
        return ctx.ring_tracks(**args)
    if method in ('contour_overturning', 'contour_interior'):
        kw.setdefault('select', 'all')
    return getattr(ctx, method)(q, contours, **kw)


_BAD, _EDGES = nat.XC_EBADARG, nat.XC_EEDGES
_Q_TEXT = 'q must be (nslab, ny, nx)'
_C_TEXT = 'contours must be (N,) or (nslab, N)'
_ASC = '%s: contours must be ascending without NaN'
_NX2 = 'xc_contour_segments_periodic: nx >= 2'
_NX3 = '%s: a periodic plane needs nx >= 3'
_BIG = '%s: plane too large for 32-bit labels (2 ny nx < 2^31)'
_SEL = '%s: select is \'all\', \'circumpolar\' or \'main\' (0, 1, 2), not %r'
_RING = '%s: select=%r needs periodic=True (no piece goes round a plain plane)'
_WT, _FT = '%s: w must be (ny, nx) or (nslab, ny, nx)', '%s: f must be (nslab, ny, nx)'
_DESC = np.where(np.arange(S)[:, None] == S - 1, -1.0, 1.0) * np.arange(3.0)       # descending in the last slab (the last batch)
_METHODS = [('contour_polylines', 'xc_contour_polylines'), ('contour_overturning', 'xc_contour_overturning'),
            ('contour_interior', 'xc_contour_interior'), ('contour_piece_interiors', 'xc_contour_piece_interiors'),
            ('contour_piece_tree', 'xc_contour_piece_tree'), ('contour_piece_labels', 'xc_contour_piece_labels'),
            ('contour_piece_props', 'xc_contour_piece_props'), ('contour_piece_overlap', 'xc_contour_piece_overlap'),
            ('contour_piece_tracks', 'xc_contour_piece_tracks')]
# (method, what is wrong, keyword arguments of _call, error code, text)
_REFUSED = []
for m, who in _METHODS:
    _REFUSED += [(m, 'q not 3-D', dict(q=np.zeros((NY, NX))), _BAD, _Q_TEXT),
                 (m, 'contours 3-D', dict(contours=np.zeros((S, 1, N))), _BAD, _C_TEXT),
                 (m, 'wrong leading contour dim', dict(contours=np.zeros((S + 1, N))), _BAD, _C_TEXT),
                 (m, 'zero contours', dict(contours=np.zeros(0)), _BAD, _C_TEXT),
                 (m, 'a NaN contour', dict(contours=np.array([0.0, np.nan, 1.0])), _EDGES, _ASC % who),
                 (m, 'a descending contour', dict(contours=np.array([0.0, 1.0, 0.5])), _EDGES, _ASC % who),
                 (m, 'a descending contour of the last slab', dict(contours=_DESC), _EDGES, _ASC % who)]
    if m not in ('contour_piece_overlap', 'contour_piece_tracks'):  # (these two stage their batch before they get that far)
        _REFUSED += [(m, 'a plane of 2^30 nodes', dict(q=_Huge()), _BAD, _BIG % who)]
    if m in ('contour_polylines', 'contour_overturning', 'contour_interior'):
        _REFUSED += [(m, 'nx == 1 on a ring', dict(q=np.zeros((S, NY, 1)), periodic=True), _BAD, _NX2)]
    else:
        _REFUSED += [(m, 'nx == 2 on a ring', dict(q=np.zeros((S, NY, 2)), periodic=True), _BAD, _NX3 % who)]
    if m in ('contour_overturning', 'contour_interior'):
        _REFUSED += [(m, 'select %r' % (s,), dict(select=s, periodic=True), _BAD, _SEL % (who, s)) for s in ('most', 3, -1, True, 1.5)]
        _REFUSED += [(m, 'select %r on a plane' % (s,), dict(select=s), _BAD, _RING % (who, s)) for s in ('main', 'circumpolar', 1, 2)]
        _REFUSED += [(m, 'a bad select before a ring too narrow', dict(q=np.zeros((S, NY, 1)), periodic=True, select='most'), _BAD,
                      _SEL % (who, 'most'))]
    if m not in ('contour_polylines', 'contour_overturning'):
        _REFUSED += [(m, 'w a row', dict(w=np.ones(NY)), _BAD, _WT % who),
                     (m, 'w for other slabs', dict(w=np.ones((S + 1, NY, NX))), _BAD, _WT % who)]
    if m not in ('contour_polylines', 'contour_overturning', 'contour_piece_props'):
        _REFUSED += [(m, 'f one plane', dict(f=np.ones((NY, NX))), _BAD, _FT % who),
                     (m, 'w bad before f bad', dict(w=np.ones(NY), f=np.ones((NY, NX))), _BAD, _WT % who)]
_P, _O, _T, _R, _L = 'contour_piece_props', 'contour_piece_overlap', 'contour_piece_tracks', 'ring_tracks', 'label_overlap'
_REFUSED += [(_P, 'nine fields', dict(fields=[W] * 9), _BAD, 'xc_contour_piece_props: 9 fields, at most 8 (XC_PROPS_MAXF)'),
             (_P, 'a field a row', dict(fields=[W, np.ones(NY)]), _BAD, 'xc_contour_piece_props: a field must be (ny, nx) or (nslab, ny, nx)'),
             (_P, 'x one plane', dict(x=W), _BAD, 'xc_contour_piece_props: x must be (nslab, ny, nx)'),
             (_P, 'w bad before nine fields', dict(w=np.ones(NY), fields=[W] * 9), _BAD, _WT % 'xc_contour_piece_props'),
             (_P, 'a ring too narrow before w bad', dict(q=np.zeros((S, NY, 2)), periodic=True, w=np.ones(NY)), _BAD,
              _NX3 % 'xc_contour_piece_props'),
             (_O, 'fields of two shapes', dict(qb=np.zeros((S, NY, NX + 1))), _BAD, 'xc_contour_piece_overlap: the two fields must have one shape'),
             (_O, 'the other field not 3-D', dict(qb=np.zeros((NY, NX))), _BAD, _Q_TEXT),
             (_O, 'contours_b of another count', dict(contours_b=np.arange(N + 1.0)), _BAD,
              'xc_contour_piece_overlap: as many levels for the one field as for the other'),
             (_O, 'contours_b 3-D', dict(contours_b=np.zeros((S, 1, N))), _BAD, _C_TEXT),
             (_O, 'descending contours_b', dict(contours_b=np.arange(N)[::-1] * 1.0), _EDGES, _ASC % 'xc_contour_piece_overlap'),
             (_T, 'min_overlap above 1', dict(min_overlap=1.5), _BAD, 'xc_contour_piece_tracks: min_overlap must lie in [0, 1]'),
             (_T, 'min_overlap below 0', dict(min_overlap=-0.1), _BAD, 'xc_contour_piece_tracks: min_overlap must lie in [0, 1]'),
             (_T, 'min_overlap NaN', dict(min_overlap=np.nan), _BAD, 'xc_contour_piece_tracks: min_overlap must lie in [0, 1]'),
             (_T, 'min_overlap bad before w bad', dict(min_overlap=2, w=np.ones(NY)), _BAD, 'xc_contour_piece_tracks: min_overlap must lie in [0, 1]'),
             (_R, 'ring_step 2-D', dict(ring_step=np.zeros((2, 2))), _BAD, 'xc_ring_tracks: ring_step (nring,), link_a, link_b and link_n (nlink,)'),
             (_R, 'link_b shorter', dict(link_b=np.zeros(2)), _BAD, 'xc_ring_tracks: ring_step (nring,), link_a, link_b and link_n (nlink,)'),
             (_R, 'link_n longer', dict(link_n=np.zeros(4)), _BAD, 'xc_ring_tracks: ring_step (nring,), link_a, link_b and link_n (nlink,)'),
             (_R, 'ring_size of another length', dict(ring_size=np.ones(5)), _BAD, 'xc_ring_tracks: ring_size must be (nring,)'),
             (_R, 'links without rings', dict(ring_step=np.zeros(0), ring_size=None), _BAD, 'xc_ring_tracks: links without rings'),
             (_L, 'maps of two shapes', dict(b=np.zeros((S, N, NY, NX + 1))), _BAD,
              'xc_label_overlap: two maps of one shape, (nrange, ny, nx) or (nslab, N, ny, nx)'),
             (_L, 'maps 2-D', dict(a=np.zeros((NY, NX)), b=np.zeros((NY, NX))), _BAD,
              'xc_label_overlap: two maps of one shape, (nrange, ny, nx) or (nslab, N, ny, nx)'),
             (_L, 'empty maps', dict(a=np.zeros((0, NY, NX)), b=np.zeros((0, NY, NX))), _BAD,
              'xc_label_overlap: two maps of one shape, (nrange, ny, nx) or (nslab, N, ny, nx)'),
             (_L, 'w a row', dict(w=np.ones(NY)), _BAD, _WT % 'xc_label_overlap'),
             (_L, 'f one plane', dict(f=W), _BAD, _FT % 'xc_label_overlap')]
# the checks that `contour_piece_overlap` and `contour_piece_tracks` reach only with their label maps allocated (and freed again)
_LATE = {(m, what) for m in (_O, _T) for what in ('a NaN contour', 'a descending contour', 'a descending contour of the last slab',
                                                   'nx == 2 on a ring', 'descending contours_b')}

# ... and those that may show only when their turn has come: a defect of the last batch alone, or of the second field's levels
_AFTER = {(_O, 'a descending contour of the last slab'), (_T, 'a descending contour of the last slab'), (_O, 'descending contours_b')}


@pytest.mark.parametrize('method,what,kw,code,text', _REFUSED, ids=['%s-%s' % r[:2] for r in _REFUSED])
def test_one_defect_one_error(ctx, q, method, what, kw, code, text):
    kw = dict(kw)
    q = kw.pop('q', q)
    ctx.max_batch_bytes = 2 * CELLS * (16 + 8 * N)                  # several batches, were the call to get that far
    with pytest.raises(nat.XContourHipError) as e:
        _call(ctx, method, q, **kw)
    assert e.value.code == code and str(e.value) == text
    assert ctx._buffers == []
    # refused before anything reached the library
    assert ctx.lib.calls == [] or (method, what) in _AFTER
    assert ctx.lib.mallocs == [] or (method, what) in _LATE


def test_the_defect_free_calls_of_the_table_pass(ctx, q):
    ctx.max_batch_bytes = 2 * CELLS * (16 + 8 * N)
    for m, _ in _METHODS:
        for periodic in (False, True):
            _call(ctx, m, q, periodic=periodic)
    _call(ctx, 'label_overlap', q)
    _call(ctx, 'ring_tracks', q)
    assert ctx._buffers == []
