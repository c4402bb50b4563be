"""xc_contour_piece_tree_dev (K19), the C entry on host records, against cptree_ref.piece_tree (sets of nodes, not the kernel's walk): the
integer fields equal, the four sums equal to the header's rule BIT FOR BIT, and K18's seven fields equal to what
xc_contour_piece_interiors_dev writes on the same records.  No tolerances.  The records are hand-built as in
test_gpu_cpinside_records.py: the restatements of K12 trace the planes of cptree_cases and noise, stored in a shuffled order.  Weights and
integrands have exponents in [-20, 20], so every term lies wholly inside its window (asserted below); the windows' edges, the cut at the
floor and the windows per slab are pinned in test_gpu_ring_sums.py.
Every call hands the entry output arrays filled with a pattern and followed by guard elements: on XC_OK the records are written and
every guard intact, on 1 or a refusal nothing but piece_count is touched."""
import numpy as np
import pytest

import cptree_cases as CS
import cptree_ref as TR
import test_gpu_cpinside_records as K18
from test_gpu_cpinside_records import DEFAULT_CAP, GUARD, scaled, shuffled, trace
from xcontour_amd import _native as nat

pytestmark = pytest.mark.gpu

I64, F64 = 0x5a5a5a5a5a5a5a5a, -1.2345e300
PATS = K18.PATS + ((np.int64, I64), (np.int32, 0x5a5a5a5a), (np.int32, 0x5a5a5a5a), (np.int64, I64), (np.float64, F64), (np.float64, F64))
NAMES = K18.NAMES + ('parent', 'depth', 'nchild', 'n_net', 'net_w', 'net_wf')


def call(ctx, count, e_from, e_to, pts, ny, nx, periodic, flip, ncont, w=None, f=None, capacity=None, null_records=False):
    """one call -> (rc, piece_count, the thirteen columns as written, untouched); the guards are checked"""
    count = np.ascontiguousarray(count, dtype=np.uint64).ravel()
    total, nr = int(count.sum()), count.size
    capacity = total if capacity is None else int(capacity)
    ins = [count, np.ascontiguousarray(e_from, dtype=np.int64), np.ascontiguousarray(e_to, dtype=np.int64),
           np.ascontiguousarray(pts, dtype=np.float64).reshape(-1)]
    opt = [np.ascontiguousarray(a) for a in (w, f) if a is not None]
    size = max(capacity, 1)
    outs = [np.full(nr + GUARD, I64, dtype=np.uint64)] + [np.full(size + GUARD, p, dtype=t) for t, p in PATS]
    w_per_slab = 1 if w is not None and np.ndim(w) == 3 else 0
    with ctx._temporaries(ins + opt + outs, []) as bufs:
        dn, df, dt, dp = bufs[:4]
        dw = bufs[4] if w is not None else None
        dfi = bufs[4 + (w is not None)] if f is not None else None
        dpc, *rec = bufs[-(len(PATS) + 1):]
        ptrs = [None] * len(PATS) if null_records else [b.ptr for b in rec]
        if f is None:
            ptrs[6] = ptrs[12] = None
        rc = ctx.lib.xc_contour_piece_tree_dev(ctx.handle, nr, dn.ptr, df.ptr, dt.ptr, dp.ptr, ny, nx, int(periodic), int(flip), int(ncont),
                                               dw.ptr if dw is not None else None, w_per_slab, dfi.ptr if dfi is not None else None,
                                               nat.dtype_code(f.dtype) if f is not None else 0, capacity, dpc.ptr, *ptrs)
        pcb = dpc.download((nr + GUARD,), np.uint64)
        back = [b.download((size + GUARD,), t) for b, (t, _) in zip(rec, PATS)]
    assert (pcb[nr:] == I64).all(), 'the guard behind piece_count was written'
    fresh = [np.full(size + GUARD, p, dtype=t) for t, p in PATS]
    npiece = int(pcb[:nr].sum()) if rc == 0 else 0
    for name, b, fr in zip(NAMES, back, fresh):
        assert b[npiece:].tobytes() == fr[npiece:].tobytes(), '%s was written behind the %d pieces' % (name, npiece)
    untouched = all(b.tobytes() == fr.tobytes() for b, fr in zip(back, fresh))
    if f is None:
        assert back[6].tobytes() == fresh[6].tobytes() and back[12].tobytes() == fresh[12].tobytes(), 'sum_wf / net_wf written without f'
    return rc, pcb[:nr].astype(np.int64), [b[:npiece] for b in back], untouched


def tables(ctx, rec, ny, nx, periodic, flip, ncont, cap=None, **kw):
    """-> per range the table (TR.DTYPE) sorted by first_edge, `parent` a row of it"""
    try:
        if cap is not None:
            ctx.set_cpiece_workspace(cap)
        rc, pc, cols, _ = call(ctx, *rec[:4], ny, nx, periodic, flip, ncont, **kw)
        groups = ctx.last_cptree_profile()['groups']
    finally:
        if cap is not None:
            ctx.set_cpiece_workspace(DEFAULT_CAP)
    assert rc == 0, 'xc_contour_piece_tree_dev returned %d' % rc
    out, p0 = [], 0
    for n in pc:
        n = int(n)
        t = np.empty(n, dtype=TR.DTYPE)
        for name, col in zip(NAMES, cols):
            t[name] = col[p0:p0 + n] if (name not in ('sum_wf', 'net_wf') or kw.get('f') is not None) else np.nan
        par = t['parent'].copy()
        assert ((par == -1) | ((par >= p0) & (par < p0 + n))).all(), 'a parent outside the range of its piece'
        order = np.argsort(t['first_edge'], kind='stable')
        where = np.empty(n, dtype=np.int64)
        where[order] = np.arange(n)
        t['parent'] = np.where(par >= 0, where[np.clip(par - p0, 0, max(n - 1, 0))], -1) if n else par
        out.append(t[order])
        p0 += n
    return out, groups


def check(ctx, rec, ny, nx, periodic, flip, ncont, what='', cap=None, w=None, f=None, tops=None):
    got, _ = tables(ctx, rec, ny, nx, periodic, flip, ncont, cap=cap, w=w, f=f)
    ref = TR.piece_tree(*rec[:4], ny, nx, periodic, flip=flip, ncont=ncont, w=w, f=f, tops=tops)
    assert len(got) == len(ref)
    for r, (g, t) in enumerate(zip(got, ref)):
        bad = TR.differences(g, t)
        assert bad == [], '%s (periodic %d, flip %d) range %d: %r differ' % (what, periodic, flip, r, bad)
    # K18's fields are what K18's entry writes on the same records
    k18 = K18.tables(ctx, rec, ny, nx, periodic, flip, ncont, w=w, f=f)
    for g, t in zip(got, k18):
        assert K18.PR.differences(g[list(K18.PR.DTYPE.names)].astype(K18.PR.DTYPE), t) == []
    return got


def same(a, b):
    return len(a) == len(b) and all(TR.differences(u, v) == [] for u, v in zip(a, b))


def plane_rec(q, periodic, seed=7):
    return shuffled(trace(q, periodic), seed)


# ------------------------------------------------------------------ the hand-built planes
@pytest.mark.parametrize('n', [13, 83])
def test_a_chain_of_square_rings(ctx, n):
    (t,) = check(ctx, plane_rec(CS.chain(n), 0), n, n, 0, 0, 1, 'chain')
    m = (n - 1) // 2
    t = t[np.argsort(t['n_in'])]
    k = np.arange(m)
    assert np.array_equal(t['n_in'], (2 * k + 1) ** 2) and np.array_equal(t['depth'], m - 1 - k)
    assert np.array_equal(t['n_net'], np.where(k > 0, (2 * k + 1) ** 2 - (2 * k - 1) ** 2, 1))


def test_stacked_siblings_and_two_unrelated_blobs(ctx):
    q = CS.stacked_siblings()
    (t,) = check(ctx, plane_rec(q, 0), *q.shape, 0, 0, 1, 'stacked siblings')
    block, upper, lower, island = (int(np.flatnonzero(t['n_in'] == n)[0]) for n in (98, 20, 9, 1))
    assert [t['parent'][k] for k in (block, upper, lower, island)] == [-1, block, block, upper] and t['nchild'][block] == 2
    q = CS.two_blobs()
    (t,) = check(ctx, plane_rec(q, 0), *q.shape, 0, 0, 1, 'two blobs')
    assert t['parent'].tolist() == [-1, -1]


@pytest.mark.parametrize('flip', [0, 1])
def test_two_rings_that_go_round_and_three_blobs(ctx, flip):
    q = CS.bands()
    (t,) = check(ctx, plane_rec(q, 1), *q.shape, 1, flip, 1, 'bands')
    assert t['parent'].tolist() == ([-1, -1, 1, 1, 3] if not flip else [1, 3, 3, -1, -1])


def test_a_ring_across_the_seam_and_the_same_field_on_a_plain_plane(ctx):
    q = CS.seam()
    for flip in (0, 1):
        (t,) = check(ctx, plane_rec(q, 1), *q.shape, 1, flip, 1, 'seam')
        assert sorted(t['depth'].tolist()) == [0, 1, 2] and sorted(t['n_net'].tolist()) == [1, 8, 33]
        (p,) = check(ctx, plane_rec(q, 0), *q.shape, 0, flip, 1, 'seam, plain')
        assert not p['closed'].any() and (p['parent'] == -1).all() and (p['n_net'] == -1).all()


@pytest.mark.parametrize('q', [CS.open_above(), CS.open_beside_nan(False), CS.open_beside_nan(True)],
                         ids=['edge to edge', 'beside a NaN cell', 'a parent behind the open piece'])
def test_open_pieces_are_transparent(ctx, q):
    for flip in (0, 1):
        (t,) = check(ctx, plane_rec(q, 0), *q.shape, 0, flip, 1, 'open piece')
        o = t[~t['closed']]
        assert o.size == 1 and (o['parent'][0], o['depth'][0], o['nchild'][0], o['n_net'][0]) == (-1, 0, 0, -1)
        assert np.isnan(o['net_w'][0])
        hole = t[t['closed'] & (t['n_in'] == 1)][0]
        assert hole['parent'] == (-1 if t.size == 2 else int(np.argmax(t['n_in'])))


def test_saddles_a_single_node_and_long_walks(ctx):
    for q, periodic in ((CS.checkerboard(), 0), (CS.one_node(), 0), (CS.long_walk(True), 1), (CS.long_walk(False), 1)):
        for flip in (0, 1):
            got = check(ctx, plane_rec(q, periodic), *q.shape, periodic, flip, 1, 'small planes')
    assert got[0]['parent'].tolist() == [-1]
    (t,) = check(ctx, plane_rec(CS.long_walk(True), 1), 600, 4, 1, 0, 1, 'long walk')
    assert t['parent'][np.argmin(t['n_in'])] == np.argmax(t['n_in']) and sorted(t['n_net'].tolist()) == [1, 3 * 598 - 1]


# ------------------------------------------------------------------ groups, slabs, weights and integrands
def noise_case(periodic):
    ny, nx = 24, 31
    q = np.stack([CS.smooth_noise(ny, nx, 40 + s) for s in range(3)])
    q[1, 5, 7] = np.nan
    lv = np.array([-0.9, -0.3, 0.2, 0.8])
    return q, shuffled(trace(q, periodic, lv), 41), ny, nx


@pytest.mark.parametrize('periodic', [0, 1], ids=['plain', 'ring'])
def test_twelve_ranges_in_one_group_and_in_many_with_every_weight_and_integrand(ctx, periodic):
    q, rec, ny, nx = noise_case(periodic)
    rng = np.random.default_rng(42)
    w2, w3 = scaled(rng, (ny, nx)), scaled(rng, (3, ny, nx))                  # negative weights among them
    f32, f64 = scaled(rng, (3, ny, nx), np.float32), scaled(rng, (3, ny, nx))
    variants = [dict(w=w2, f=f64), dict(w=w3, f=f32), dict(w=None, f=None), dict(w=None, f=f64)]
    one_row = 2 * ny * nx * 4
    for k, flip in enumerate((0, 1, 1, 0)):
        v = variants[(k + periodic) % 4]
        got = check(ctx, rec, ny, nx, periodic, flip, 4, 'noise', **v)
        for cap, least in ((4 * one_row, 3), (1, 4)):                         # four ranges per group at most; one range per group
            again, groups = tables(ctx, rec, ny, nx, periodic, flip, 4, cap=cap, **v)
            assert groups >= least and same(again, got), 'the groups show (cap %d)' % cap
        # inside their windows the sums are plain math.fsum
        ref, masks = TR.piece_tree(*rec, ny, nx, periodic, flip=flip, ncont=4, return_masks=True, **v)
        for r, (t, ms) in enumerate(zip(ref, masks)):
            ws, wf = TR.IR.slab_planes(v['w'], v['f'], r // 4, ny, nx)
            for p in np.flatnonzero(t['closed']):
                net = ms[p].copy()
                for c in np.flatnonzero(t['parent'] == p):
                    net &= ~ms[c]
                assert TR.IR.same_bits(np.array([got[r]['net_w'][p]]), np.array([TR.IR.nan_skipping_sum(ws[net])]))
                if wf is not None:
                    assert TR.IR.same_bits(np.array([got[r]['net_wf'][p]]), np.array([TR.IR.nan_skipping_sum(wf[net])]))
    assert max(int(t['depth'].max()) for t in got if t.size) >= 1 and any((~t['closed']).any() for t in got)


def test_an_infinite_weight_inside_a_child_poisons_the_parent_gross_and_net_and_not_the_sibling(ctx):
    q = CS.stacked_siblings()
    ny, nx = q.shape
    rng = np.random.default_rng(43)
    w, f = scaled(rng, (ny, nx)), scaled(rng, (1, ny, nx))
    w[5, 3] = np.inf                                                         # the island in the upper hole
    w[11, 4] = np.nan                                                        # skipped in the lower hole
    (t,) = check(ctx, plane_rec(q, 0), ny, nx, 0, 0, 1, 'inf in a child', w=w, f=f)
    block, upper, lower, island = (int(np.flatnonzero(t['n_in'] == n)[0]) for n in (98, 20, 9, 1))
    for k in (block, upper, island):
        assert all(np.isnan(t[name][k]) for name in ('sum_w', 'net_w', 'sum_wf', 'net_wf'))
    assert all(np.isfinite(t[name][lower]) for name in ('sum_w', 'net_w', 'sum_wf', 'net_wf'))


# ------------------------------------------------------------------ the capacity protocol
def test_the_capacity_protocol(ctx):
    q, rec, ny, nx = noise_case(0)
    npiece = [t.size for t in TR.PR.piece_interiors(*rec, ny, nx, 0, ncont=4)]
    for cap in (None, 1):
        try:
            if cap is not None:
                ctx.set_cpiece_workspace(cap)
            rc, pc, _, untouched = call(ctx, *rec, ny, nx, 0, 0, 4, capacity=0, null_records=True)
            assert rc == 1 and pc.tolist() == npiece and untouched, 'count only'
            rc, pc, _, untouched = call(ctx, *rec, ny, nx, 0, 0, 4, capacity=sum(npiece) - 1)
            assert rc == 1 and pc.tolist() == npiece and untouched, 'one record short'
            rc, pc, cols, _ = call(ctx, *rec, ny, nx, 0, 0, 4, capacity=sum(npiece))
            assert rc == 0 and pc.tolist() == npiece and cols[7].size == sum(npiece), 'an exact fit'
        finally:
            ctx.set_cpiece_workspace(DEFAULT_CAP)
    rc, _, _, untouched = call(ctx, *rec, ny, nx, 0, 2, 4)
    assert rc == nat.XC_EBADARG and untouched, 'flip 2'
