"""xc_contour_piece_labels_dev (K20), the C entry on host records, against cplabel_ref.labels_of_masks (sets of nodes, not the kernel's
scan): every label equal, and K19's thirteen columns equal BIT FOR BIT to what xc_contour_piece_tree_dev writes on the same records.  No
tolerances.  The records are hand-built as in test_gpu_cptree_records.py: the restatements of K12 trace the planes of cptree_cases and
noise, stored in an order of the test's choosing.  Every call hands the entry a map filled with a pattern, with guard elements before
and behind it: on XC_OK every element of the map is written and every guard intact."""
import numpy as np
import pytest

import cplabel_ref as LR
import cpiece_records_ref as RR
import cptree_cases as CS
import cptree_ref as TR
import test_gpu_cptree_records as K19
from test_cplabel_host import PLANES
from test_gpu_cpiece_records import run_records as k13_tables
from test_gpu_cpinside_records import DEFAULT_CAP, GUARD, scaled, shuffled, stored, trace
from xcontour_amd import _native as nat

pytestmark = pytest.mark.gpu

PATS, NAMES = K19.PATS, K19.NAMES
LPAT = 0x5a5a5a5a


def call(ctx, count, e_from, e_to, pts, ny, nx, periodic, flip, ncont, w=None, f=None, capacity=None, null_records=False,
         null_label=False):
    """one call -> (rc, piece_count, the thirteen columns as written, the map (nrange, ny, nx) as it came back); the guards are checked"""
    count = np.ascontiguousarray(count, dtype=np.uint64).ravel()
    total, nr = int(count.sum()), count.size
    capacity = total if capacity is None else int(capacity)
    ins = [count, np.ascontiguousarray(e_from, dtype=np.int64), np.ascontiguousarray(e_to, dtype=np.int64),
           np.ascontiguousarray(pts, dtype=np.float64).reshape(-1)]
    ins = [a if a.size else np.zeros(1, dtype=a.dtype) for a in ins]          # (a call without any segment)
    opt = [np.ascontiguousarray(a) for a in (w, f) if a is not None]
    size, nmap = max(capacity, 1), nr * max(ny, 1) * max(nx, 1)
    outs = [np.full(nr + GUARD, K19.I64, dtype=np.uint64)] + [np.full(size + GUARD, p, dtype=t) for t, p in PATS]
    outs.append(np.full(nmap + 2 * GUARD, LPAT, dtype=np.int32))
    w_per_slab = 1 if w is not None and np.ndim(w) == 3 else 0
    with ctx._temporaries(ins + opt + outs, []) as bufs:
        dn, df, dt, dp = bufs[:4]
        dw = bufs[4] if w is not None else None
        dfi = bufs[4 + (w is not None)] if f is not None else None
        dpc, *rec, dlab = bufs[-(len(PATS) + 2):]
        ptrs = [None] * len(PATS) if null_records else [b.ptr for b in rec]
        if f is None:
            ptrs[6] = ptrs[12] = None
        rc = ctx.lib.xc_contour_piece_labels_dev(ctx.handle, nr, dn.ptr, df.ptr, dt.ptr, dp.ptr, ny, nx, int(periodic), int(flip), int(ncont),
                                                 dw.ptr if dw is not None else None, w_per_slab, dfi.ptr if dfi is not None else None,
                                                 nat.dtype_code(f.dtype) if f is not None else 0, capacity, dpc.ptr, *ptrs,
                                                 None if null_label else dlab.ptr + 4 * GUARD)
        pcb = dpc.download((nr + GUARD,), np.uint64)
        back = [b.download((size + GUARD,), t) for b, (t, _) in zip(rec, PATS)]
        lab = dlab.download((nmap + 2 * GUARD,), np.int32)
    assert (pcb[nr:] == K19.I64).all(), 'the guard behind piece_count was written'
    assert (lab[:GUARD] == LPAT).all() and (lab[GUARD + nmap:] == LPAT).all(), 'a guard of the map was written'
    fresh = [np.full(size + GUARD, p, dtype=t) for t, p in PATS]
    npiece = int(pcb[:nr].sum()) if rc == 0 else 0
    for name, b, fr in zip(NAMES, back, fresh):
        assert b[npiece:].tobytes() == fr[npiece:].tobytes(), '%s was written behind the %d pieces' % (name, npiece)
    if rc != 0:
        assert all(b.tobytes() == fr.tobytes() for b, fr in zip(back, fresh)), 'a record array was written without XC_OK'
    return rc, pcb[:nr].astype(np.int64), [b[:npiece] for b in back], lab[GUARD:GUARD + nmap].reshape(nr, ny, nx)


def results(ctx, rec, ny, nx, periodic, flip, ncont, cap=None, **kw):
    """-> (per range the table (TR.DTYPE) sorted by first_edge, per range the map in rows of that table, the groups of the call)"""
    try:
        if cap is not None:
            ctx.set_cpiece_workspace(cap)
        rc, pc, cols, lab = call(ctx, *rec[:4], ny, nx, periodic, flip, ncont, **kw)
        groups = ctx.last_cplabel_profile()['groups']
    finally:
        if cap is not None:
            ctx.set_cpiece_workspace(DEFAULT_CAP)
    assert rc == 0, 'xc_contour_piece_labels_dev returned %d' % rc
    assert (lab != LPAT).all(), 'the map is not fully written'
    tabs, maps, p0 = [], [], 0
    for r, n in enumerate(pc):
        n = int(n)
        t = np.empty(n, dtype=TR.DTYPE)
        for name, col in zip(NAMES, cols):
            t[name] = col[p0:p0 + n] if (name not in ('sum_wf', 'net_wf') or kw.get('f') is not None) else np.nan
        par = t['parent'].copy()
        order = np.argsort(t['first_edge'], kind='stable')
        where = np.empty(n, dtype=np.int64)
        where[order] = np.arange(n)
        t['parent'] = np.where(par >= 0, where[np.clip(par - p0, 0, max(n - 1, 0))], -1) if n else par
        assert lab[r].min() >= -1 and lab[r].max() < max(n, 1), 'a label outside the pieces of its range'
        maps.append(np.where(lab[r] >= 0, where[np.maximum(lab[r], 0)], -1).astype(np.int32) if n else lab[r])
        tabs.append(t[order])
        p0 += n
    return tabs, maps, groups


def check(ctx, rec, ny, nx, periodic, flip, ncont, what='', cap=None, w=None, f=None):
    tabs, maps, _ = results(ctx, rec, ny, nx, periodic, flip, ncont, cap=cap, w=w, f=f)
    ref, masks = TR.piece_tree(*rec[:4], ny, nx, periodic, flip=flip, ncont=ncont, w=w, f=f, return_masks=True)
    assert len(tabs) == len(ref)
    for r, (g, t, m, ms) in enumerate(zip(tabs, ref, maps, masks)):
        where = '%s (periodic %d, flip %d) range %d' % (what, periodic, flip, r)
        assert TR.differences(g, t) == [], where
        assert np.array_equal(m, LR.labels_of_masks(ms, (ny, nx))), where
        assert np.array_equal(np.bincount(m[m >= 0], minlength=g.size)[g['closed']], g['n_net'][g['closed']]), where
    # K19's columns are what K19's entry writes on the same records
    k19, _ = K19.tables(ctx, rec, ny, nx, periodic, flip, ncont, w=w, f=f)
    for g, t in zip(tabs, k19):
        assert g.tobytes() == t.tobytes()
    return tabs, maps


def orders(rec):
    """the records in three storage orders: two shuffles and every range reversed"""
    return (shuffled(rec, 7), shuffled(rec, 8), stored(rec, [np.arange(int(c))[::-1] for c in rec[0].ravel()]))


# ------------------------------------------------------------------ the hand-built planes
@pytest.mark.parametrize('name, q, periodic', PLANES, ids=[p[0] for p in PLANES])
def test_every_hand_built_plane_in_three_storage_orders_under_two_caps(ctx, name, q, periodic):
    ny, nx = q.shape
    first = {}
    for flip in (0, 1):
        for k, rec in enumerate(orders(trace(q, periodic))):
            for cap in (None, 1) if k == 0 else (None,):
                (t,), (m,) = check(ctx, rec, ny, nx, periodic, flip, 1, name, cap=cap)
                assert np.array_equal(m, first.setdefault(flip, m)), 'the storage order or the cap shows'
        if t['closed'].any():
            assert (m >= 0).any()
        if name in ('chain 13', 'chain 83', 'seam'):
            assert t['depth'].max() >= 2 and (m == -1).any()
        if name in ('seam, plain', 'open above', 'open beside NaN', 'open beside NaN, enclosed'):
            assert (~t['closed']).any() and not np.isin(m, np.flatnonzero(~t['closed'])).any()
    assert LR.scan_geometry(ny)[1] == {600: 32, 83: 6}.get(ny, 1)            # the row-chunk regimes these planes run in


# ------------------------------------------------------------------ groups, slabs, weights and integrands
@pytest.mark.parametrize('periodic', [0, 1], ids=['plain', 'ring'])
def test_twelve_ranges_in_one_group_and_in_many_with_weights_and_integrands(ctx, periodic):
    q, rec, ny, nx = K19.noise_case(periodic)
    rng = np.random.default_rng(42)
    variants = [dict(w=scaled(rng, (ny, nx)), f=scaled(rng, (3, ny, nx))), dict(w=scaled(rng, (3, ny, nx)), f=scaled(rng, (3, ny, nx), np.float32)),
                dict(w=None, f=None)]
    one_row = 2 * ny * nx * 4
    for k, flip in enumerate((0, 1, 1)):
        v = variants[(k + periodic) % 3]
        tabs, maps = check(ctx, rec, ny, nx, periodic, flip, 4, 'noise', **v)
        for cap, least in ((4 * one_row, 3), (1, 4)):                         # four ranges per group at most; one range per group
            t2, m2, groups = results(ctx, rec, ny, nx, periodic, flip, 4, cap=cap, **v)
            assert groups >= least and K19.same(t2, tabs) and all(np.array_equal(a, b) for a, b in zip(m2, maps)), 'the groups show'
    assert max(int(t['depth'].max()) for t in tabs if t.size) >= 1 and any((~t['closed']).any() for t in tabs)
    assert any((m >= 0).any() and (m == -1).any() for m in maps) and LR.scan_geometry(ny) == (16, 2)


# ------------------------------------------------------------------ geometry
@pytest.mark.parametrize('ny, nx', [(24, 63), (24, 64), (24, 65), (6, 255), (6, 256), (6, 257), (17, 33), (83, 20), (513, 5)])
def test_columns_on_both_sides_of_a_wave_and_of_a_block_and_every_row_chunk_regime(ctx, ny, nx):
    """ny 6: one chunk; 17: a second chunk of one row; 24: two chunks; 83: six chunks of 16 rows, the last one short; 513: 31 chunks of
    17 rows (the chunks grow once there would be more than 32)"""
    assert LR.scan_geometry(ny) == {6: (16, 1), 17: (16, 2), 24: (16, 2), 83: (16, 6), 513: (17, 31)}[ny]
    q = CS.smooth_noise(ny, nx, ny + nx)[None]
    if ny == 17:
        q[0, 2:15, 10:23] = 4.0 * CS.chain(13) - 2.0                        # (so few rows of noise hold no ring in a ring)
    q[0, ny // 2, nx // 3] = np.nan
    lv = np.array([-0.4, 0.5])
    deep = 0
    for periodic in (0, 1):
        rec = shuffled(trace(q, periodic, lv), 11)
        for flip in (0, 1):
            tabs, maps = check(ctx, rec, ny, nx, periodic, flip, 2, 'geometry')
            deep = max(deep, max(int(t['depth'].max()) for t in tabs if t.size))
            assert any((m >= 0).any() and (m == -1).any() for m in maps)
    assert deep >= 1 or ny == 6


def test_one_edge_row(ctx):
    q = np.zeros((2, 9))
    q[1, 3:6] = 1.0                                                          # ones on the last row: an open piece on a plain plane
    for periodic in (0, 1):
        for flip in (0, 1):
            (t,), (m,) = check(ctx, shuffled(trace(q, periodic), 3), 2, 9, periodic, flip, 1, 'ny 2')
            assert t.size == 1 and not t['closed'][0] and (m == -1).all()
    q = np.zeros((2, 9))
    q[1] = 1.0                                                               # a ring that goes round, one crossing per column
    for flip in (0, 1):
        (t,), (m,) = check(ctx, shuffled(trace(q, 1), 3), 2, 9, 1, flip, 1, 'ny 2, a ring round')
        assert t['closed'][0] and t['winding'][0] != 0 and (m[0 if flip else 1] == 0).all() and (m[1 if flip else 0] == -1).all()


def test_ranges_without_segments_are_all_minus_one_wherever_they_lie(ctx):
    ny, nx = 24, 31
    q = np.stack([CS.smooth_noise(ny, nx, 40 + s) for s in range(2)])
    lv = np.array([-99.0, -0.3, 50.0, 60.0, 0.4, 99.0])                       # empty ranges in front, between and behind
    rec = shuffled(trace(q, 1, lv), 5)
    assert (rec[0].reshape(2, 6) > 0).tolist() == [[False, True, False, False, True, False]] * 2
    for cap in (None, 1):
        tabs, maps = check(ctx, rec, ny, nx, 1, 0, 6, 'empty ranges', cap=cap)
        assert all((maps[r] == -1).all() for r in (0, 2, 3, 5, 6, 8, 9, 11)) and all((maps[r] >= 0).any() for r in (1, 4, 7, 10))
    # a call without any segment: XC_OK, nothing but -1, with and without room for records
    none = (np.zeros(3, dtype=np.uint64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros((0, 4)))
    for capacity, null in ((4, False), (0, True)):
        rc, pc, cols, lab = call(ctx, *none, ny, nx, 0, 1, 3, capacity=capacity, null_records=null)
        assert rc == 0 and pc.tolist() == [0, 0, 0] and (lab == -1).all()


# ------------------------------------------------------------------ the capacity protocol and the refusals
def test_the_capacity_protocol_and_the_refusals(ctx):
    q, rec, ny, nx = K19.noise_case(0)
    npiece = [t.size for t in TR.PR.piece_interiors(*rec, ny, nx, 0, ncont=4)]
    for cap in (None, 1):
        try:
            if cap is not None:
                ctx.set_cpiece_workspace(cap)
            rc, pc, _, _ = call(ctx, *rec, ny, nx, 0, 0, 4, capacity=0, null_records=True, null_label=True)
            assert rc == 1 and pc.tolist() == npiece, 'count only'
            rc, pc, _, _ = call(ctx, *rec, ny, nx, 0, 0, 4, capacity=sum(npiece) - 1)
            assert rc == 1 and pc.tolist() == npiece, 'one record short'
            rc, pc, cols, lab = call(ctx, *rec, ny, nx, 0, 0, 4, capacity=sum(npiece))
            assert rc == 0 and pc.tolist() == npiece and cols[7].size == sum(npiece) and (lab != LPAT).all(), 'an exact fit'
        finally:
            ctx.set_cpiece_workspace(DEFAULT_CAP)
    rc, _, _, lab = call(ctx, *rec, ny, nx, 0, 0, 4, null_label=True)
    assert rc == nat.XC_EBADARG and (lab == LPAT).all(), 'label NULL with capacity > 0'
    for a_ny, a_nx, periodic, flip, ncont in ((ny, nx, 0, 2, 4), (ny, nx, 0, 0, 5), (ny, 2, 1, 0, 4)):   # K19's refusals
        rc, _, _, lab = call(ctx, *rec, a_ny, a_nx, periodic, flip, ncont)
        assert rc == nat.XC_EBADARG and (lab == LPAT).all(), (a_ny, a_nx, periodic, flip, ncont)


def test_k13_finds_a_clean_table_afterwards(ctx):
    ny, nx = 40, 65
    q = np.random.default_rng(93).integers(-3, 4, (1, ny, nx)).astype(np.float64)
    rec = shuffled(trace(q, 0, (0.0,)), 94)
    tabs, maps = check(ctx, rec, ny, nx, 0, 0, 1, 'integer noise')
    assert tabs[0]['depth'].max() >= 1 and (maps[0] >= 0).any() and (maps[0] == -1).any()
    y, x = np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64)
    k13 = k13_tables(ctx, *rec, ny, nx, y, x)
    ref13 = RR.pieces(*rec, ny, nx, y, x)
    assert all(np.array_equal(g[k], t[0][k]) for g, t in zip(k13, ref13) for k in RR.INT_FIELDS)
    again, maps2 = check(ctx, rec, ny, nx, 0, 0, 1, 'the call after K13')
    assert K19.same(again, tabs) and np.array_equal(maps2[0], maps[0])
