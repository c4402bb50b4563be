"""xc_label_overlap_dev (K22), the C entry on hand-built maps, against cpoverlap_ref.overlap_of_maps (np.unique over the pairs, not the
kernel's walk): a, b and n equal, sum_w and sum_wf BIT FOR BIT the math.fsum of the terms.  No tolerances.  Every call hands the entry
arrays filled with a pattern, with guard elements before and behind each of them: on XC_OK exactly the rows are written, otherwise
nothing, and every guard is intact."""
import numpy as np
import pytest

import cpoverlap_ref as OR
from xcontour_amd import _native as nat

pytestmark = pytest.mark.gpu

GUARD = 16
DEFAULT_CAP = 1 << 30
I32, I64, F64 = 0x5a5a5a5a, 0x5a5a5a5a5a5a5a5a, -1.2345e300
PATS = ((np.int32, I32), (np.int32, I32), (np.int64, I64), (np.float64, F64), (np.float64, F64))
NAMES = ('a', 'b', 'n', 'sum_w', 'sum_wf')
CASES = OR.cases()


def call(ctx, la, lb, ncont=1, w=None, f=None, capacity=None, null_rows=False, null_a=False, ny=None, nx=None):
    """one call -> (rc, pair_count, the five columns as written); the guards are checked.  capacity None: what a count-only call asks for"""
    la, lb = np.ascontiguousarray(la, dtype=np.int32), np.ascontiguousarray(lb, dtype=np.int32)
    nr = la.shape[0]
    ny, nx = la.shape[1] if ny is None else ny, la.shape[2] if nx is None else nx
    if capacity is None:
        rc, pc, _ = call(ctx, la, lb, ncont, w, f, capacity=0, null_rows=True, ny=ny, nx=nx)
        assert rc == (1 if pc.sum() else 0), 'the count-only call returned %d' % rc
        capacity = int(pc.sum())
    opt = [np.ascontiguousarray(a) for a in (w, f) if a is not None]
    size = max(capacity, 1)
    outs = [np.full(nr + 2 * GUARD, I64, dtype=np.uint64)] + [np.full(size + 2 * GUARD, p, dtype=t) for t, p in PATS]
    w_per_slab = 1 if w is not None and np.ndim(w) == 3 else 0
    with ctx._temporaries([la, lb] + opt + outs, []) as bufs:
        dw = bufs[2] if w is not None else None
        dfi = bufs[2 + (w is not None)] if f is not None else None
        dpc, *rec = bufs[-(len(PATS) + 1):]
        ptrs = [None] * len(PATS) if null_rows else [b.ptr + GUARD * np.dtype(t).itemsize for b, (t, _) in zip(rec, PATS)]
        if f is None:
            ptrs[4] = None
        if null_a:
            ptrs[0] = None
        rc = ctx.lib.xc_label_overlap_dev(ctx.handle, nr, ny, nx, int(ncont), bufs[0].ptr, bufs[1].ptr, dw.ptr if dw is not None else None,
                                          w_per_slab, dfi.ptr if dfi is not None else None, nat.dtype_code(f.dtype) if f is not None else 0,
                                          capacity, dpc.ptr + 8 * GUARD, *ptrs)
        pcb = dpc.download((nr + 2 * GUARD,), np.uint64)
        back = [b.download((size + 2 * GUARD,), t) for b, (t, _) in zip(rec, PATS)]
    assert (pcb[:GUARD] == I64).all() and (pcb[GUARD + nr:] == I64).all(), 'a guard of pair_count was written'
    pc = pcb[GUARD:GUARD + nr].astype(np.int64)
    nrow = int(pc.sum()) if rc == 0 else 0
    for name, b, (t, p) in zip(NAMES, back, PATS):
        fresh = np.full(size + 2 * GUARD, p, dtype=t)
        keep = nrow if (name != 'sum_wf' or f is not None) else 0
        assert b[:GUARD].tobytes() == fresh[:GUARD].tobytes(), 'the guard before %s was written' % name
        assert b[GUARD + keep:].tobytes() == fresh[GUARD + keep:].tobytes(), '%s was written behind the %d rows' % (name, keep)
        if rc == 0 and keep and t is not np.float64:
            assert (b[GUARD:GUARD + keep] != p).all(), '%s is not fully written' % name
    return rc, pc, [b[GUARD:GUARD + nrow] for b in back]


def rows(ctx, la, lb, ncont=1, w=None, f=None, cap=None):
    """-> (per range the rows (OR.DTYPE) sorted by (a, b), the groups of the call)"""
    try:
        if cap is not None:
            ctx.set_cpiece_workspace(cap)
        rc, pc, cols = call(ctx, la, lb, ncont, w, f)
        prof = ctx.last_cpoverlap_profile()
    finally:
        if cap is not None:
            ctx.set_cpiece_workspace(DEFAULT_CAP)
    assert rc == 0, 'xc_label_overlap_dev returned %d' % rc
    assert prof['rounds'] == 0
    out, p0 = [], 0
    for n in pc.tolist():
        t = np.empty(n, dtype=OR.DTYPE)
        for name, col in zip(NAMES, cols):
            t[name] = col[p0:p0 + n] if (name != 'sum_wf' or f is not None) else np.nan
        out.append(t[np.lexsort((t['b'], t['a']))])
        p0 += n
    return out, prof['groups']


def reference(la, lb, ncont=1, w=None, f=None, tops=None):
    """tops: per slab the windows (top_w, top_f) the sums are cut in (None: no term is cut)"""
    la, lb = np.asarray(la), np.asarray(lb)
    return [OR.overlap_of_maps(la[r], lb[r], None if w is None else (w[r // ncont] if np.ndim(w) == 3 else w),
                               None if f is None else f[r // ncont], tops=None if tops is None else tops[r // ncont])
            for r in range(la.shape[0])]


def check(ctx, la, lb, ncont=1, w=None, f=None, cap=None, what='', tops=None):
    got, groups = rows(ctx, la, lb, ncont, w, f, cap)
    ref = reference(la, lb, ncont, w, f, tops)
    for r, (g, t) in enumerate(zip(got, ref)):
        assert OR.same(g, t), '%s range %d' % (what, r)
        for key, m in (('a', la[r]), ('b', lb[r])):                          # the marginals: np.bincount of the map
            m = np.asarray(m)
            lab, cnt = np.unique(m[m >= 0], return_counts=True)
            have = g[key] >= 0
            sums = {int(v): int(g['n'][have & (g[key] == v)].sum()) for v in np.unique(g[key][have]).tolist()}
            assert sums == dict(zip(lab.tolist(), cnt.tolist())), '%s range %d: the marginal of %s' % (what, r, key)
    return got, groups


# ------------------------------------------------------------------ the hand-built maps
@pytest.mark.parametrize('name', list(CASES))
def test_every_hand_built_case_twice(ctx, name):
    la, lb, w, f = CASES[name]
    f3 = None if f is None else f[None]
    got, _ = check(ctx, la[None], lb[None], 1, w, f3, what=name)
    again, _ = rows(ctx, la[None], lb[None], 1, w, f3)
    assert again[0].tobytes() == got[0].tobytes(), 'two calls differ'
    n = got[0].size
    if name == 'both all -1':
        assert n == 0
    if name == 'identical maps':
        assert n > 3 and (got[0]['a'] == got[0]['b']).all()
    if name == 'stripes':
        assert n == 4225 and (got[0]['n'] == 1).all()
    if name == 'one pair but one node':
        assert got[0][['a', 'b', 'n']].tolist() == [(3, 5, 70 * 130 - 1), (3, 6, 1)]
    if name == 'labels 2^31 - 1 and 0':
        assert (got[0]['a'] == 2 ** 31 - 1).any() and (got[0]['a'] == 0).any()
    if name == 'labels -7 and INT32_MIN':
        assert got[0]['a'].min() == -1 and got[0]['b'].min() == -1 and not ((got[0]['a'] == -1) & (got[0]['b'] == -1)).any()


@pytest.mark.parametrize('ny', [1, 16, 17, 33])
def test_rows_on_both_sides_of_a_chunk_and_columns_on_both_sides_of_a_wave(ctx, ny):
    """ny 1 and 16: one chunk; 17: a second chunk of one row; 33: a third; nx 63, 64, 65: a wave with an idle lane, a full wave, a second"""
    rng = np.random.default_rng(2210 + ny)
    for nx in (1, 63, 64, 65):
        la = np.stack([OR.blobs(rng, ny, nx, 5, fill=0.9), np.full((ny, nx), 2, dtype=np.int32)])
        lb = np.stack([OR.blobs(rng, ny, nx, 4, fill=0.9), np.full((ny, nx), -1, dtype=np.int32)])
        lb[1, ny // 2, nx // 2] = 0
        got, _ = check(ctx, la, lb, 2, OR.scaled(rng, (ny, nx)), OR.scaled(rng, (1, ny, nx)), what='%d x %d' % (ny, nx))
        assert got[1].size == (2 if ny * nx > 1 else 1)


# ------------------------------------------------------------------ slabs, weights, integrands and groups
def test_six_ranges_of_two_slabs_every_weight_and_integrand_in_one_group_and_in_many(ctx):
    ny, nx = 40, 70
    rng = np.random.default_rng(2220)
    la = np.stack([OR.blobs(rng, ny, nx, 3 + r) for r in range(6)])
    lb = np.stack([OR.blobs(rng, ny, nx, 8 - r) for r in range(6)])
    la[4], lb[4] = -1, -1                                                     # a range without rows between the others
    variants = [dict(w=OR.scaled(rng, (ny, nx)), f=OR.scaled(rng, (2, ny, nx))),
                dict(w=OR.scaled(rng, (2, ny, nx)), f=OR.scaled(rng, (2, ny, nx), np.float32)),
                dict(w=OR.scaled(rng, (2, ny, nx)), f=None), dict(w=None, f=None)]
    for v in variants:
        got, groups = check(ctx, la, lb, 3, what='six ranges', **v)
        assert groups == 1 and got[4].size == 0 and all(g.size > 3 for k, g in enumerate(got) if k != 4)
        small, many = rows(ctx, la, lb, 3, cap=1, **v)                        # one range per group
        assert many == 5 and all(a.tobytes() == b.tobytes() for a, b in zip(small, got)), 'the groups show'
    # a cap of the largest table (104 bytes a slot, the power of two >= twice the runs of 16-row chunks): it holds any one range and
    # never all five
    largest = max(1 << (2 * OR.count_runs(la[r], lb[r], 16) - 1).bit_length() for r in range(6) if r != 4)
    some, groups = rows(ctx, la, lb, 3, cap=104 * largest, **variants[0])
    assert 2 <= groups <= 5 and all(OR.same(a, b) for a, b in zip(some, reference(la, lb, 3, **variants[0])))


def test_a_nan_term_is_skipped_and_an_infinite_one_poisons_that_sum_of_that_pair_alone(ctx):
    ny, nx = 20, 66
    la, lb = np.zeros((1, ny, nx), dtype=np.int32), np.zeros((1, ny, nx), dtype=np.int32)
    lb[0, :, 30:] = 1
    lb[0, 10:, 50:] = 2
    rng = np.random.default_rng(2230)
    w, f = OR.scaled(rng, (ny, nx)), OR.scaled(rng, (1, ny, nx))
    w[3, 3] = np.nan                                                          # pair (0, 0): the term is skipped in both sums
    f[0, 4, 40] = np.inf                                                      # pair (0, 1): sum_wf NaN, sum_w not
    w[15, 60] = -np.inf                                                       # pair (0, 2): both NaN
    f[0, 5, 5] = np.nan                                                       # pair (0, 0): skipped in sum_wf alone
    (got,), _ = check(ctx, la, lb, 1, w, f, what='not finite')
    assert got['b'].tolist() == [0, 1, 2] and got['n'].tolist() == [20 * 30, 20 * 36 - 10 * 16, 10 * 16]
    assert np.isnan(got['sum_w']).tolist() == [False, False, True] and np.isnan(got['sum_wf']).tolist() == [False, True, True]


# ------------------------------------------------------------------ the capacity protocol and the refusals
def test_the_capacity_protocol_and_the_refusals(ctx):
    la, lb, w, f = CASES['blobs']
    la, lb, f = np.stack([la, lb]), np.stack([lb, la]), np.stack([f, f])
    npair = [t.size for t in reference(la, lb, 1, w, f)]
    for cap in (None, 1):
        try:
            if cap is not None:
                ctx.set_cpiece_workspace(cap)
            rc, pc, _ = call(ctx, la, lb, 1, w, f, capacity=0, null_rows=True)
            assert rc == 1 and pc.tolist() == npair, 'count only'
            rc, pc, _ = call(ctx, la, lb, 1, w, f, capacity=sum(npair) - 1)
            assert rc == 1 and pc.tolist() == npair, 'one row short'
            rc, pc, cols = call(ctx, la, lb, 1, w, f, capacity=sum(npair))
            assert rc == 0 and pc.tolist() == npair and cols[0].size == sum(npair), 'an exact fit'
            rc, pc, cols = call(ctx, la, lb, 1, w, f, capacity=sum(npair) + 7)
            assert rc == 0 and pc.tolist() == npair and cols[0].size == sum(npair), 'room to spare'
        finally:
            ctx.set_cpiece_workspace(DEFAULT_CAP)
    rc, _, _ = call(ctx, la, lb, 1, w, f, capacity=sum(npair), null_a=True)
    assert rc == nat.XC_EBADARG, 'a NULL with capacity > 0'
    rc, _, _ = call(ctx, la, lb, 1, w, None, capacity=sum(npair))
    assert rc == 0, 'sum_wf NULL without f'
    for ncont, ny, nx in ((3, 40, 70), (0, 40, 70), (1, 0, 70), (1, 40, 0)):
        rc, _, _ = call(ctx, la, lb, ncont, w if ny and nx else None, None, capacity=sum(npair), ny=ny, nx=nx)
        assert rc == nat.XC_EBADARG, (ncont, ny, nx)
    none = np.full((3, 8, 9), -1, dtype=np.int32)                            # no rows at all: XC_OK with and without room
    for capacity, null in ((4, False), (0, True)):
        rc, pc, cols = call(ctx, none, none, 3, capacity=capacity, null_rows=null)
        assert rc == 0 and pc.tolist() == [0, 0, 0]
