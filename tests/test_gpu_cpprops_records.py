"""xc_contour_piece_props_dev (K21), the C entry on host records, against cpprops_ref.piece_props (sets of nodes and math.fsum, not the
kernel's scan): every place equal, every sum and extremum equal BIT FOR BIT, and K19's thirteen columns equal byte for byte to what
xc_contour_piece_tree_dev writes on the same records.  No tolerances.  The records are hand-built as in test_gpu_cplabel_records.py.  Weights
and fields come from `scaled` (exponents in [-20, 20]): every term lies wholly inside its 160-bit window; the windows' edges, the window per
(slab, field), the wave sums and the fold at full mantissas are pinned in test_gpu_ring_sums.py.
Every call hands the entry its outputs filled with a pattern and followed by guard elements: on XC_OK nothing is written behind the
pieces of any column, on 1 or a refusal nothing but piece_count is touched."""
import numpy as np
import pytest

import cplabel_ref as LR
import cpiece_records_ref as RR
import cpprops_ref as QR
import cptree_cases as CS
import cptree_ref as TR
import test_gpu_cptree_records as K19
from test_cplabel_host import PLANES
from test_gpu_cpiece_records import run_records as k13_tables
from test_gpu_cpinside_records import DEFAULT_CAP, GUARD, scaled, shuffled, stored, trace
from xcontour_amd import _native as nat

pytestmark = pytest.mark.gpu

PATS, NAMES = K19.PATS, K19.NAMES
F64, I64 = K19.F64, K19.I64
# K21's six outputs: (name, dtype, pattern, per field)
OUTS = (('net_g', np.float64, F64, True), ('sum_g', np.float64, F64, True), ('x_min', np.float64, F64, False), ('x_max', np.float64, F64, False),
        ('at_min', np.int64, I64, False), ('at_max', np.int64, I64, False))


def call(ctx, count, e_from, e_to, pts, ny, nx, periodic, flip, ncont, w=None, fields=(), x=None, capacity=None, null_records=False,
         nf=None, null=(), g_dtype=None, x_dtype=None, null_g=None):
    """one call -> (rc, piece_count, the thirteen columns as written, K21's six outputs as written: per field (nf, npiece)); the guards
    and everything behind the pieces are checked.  nf, g_dtype, x_dtype: what the entry is TOLD; null: names of OUTS handed over as NULL;
    null_g: the field whose plane is handed over as NULL"""
    count = np.ascontiguousarray(count, dtype=np.uint64).ravel()
    total, nr = int(count.sum()), count.size
    capacity = total if capacity is None else int(capacity)
    ins = [count, np.ascontiguousarray(e_from, dtype=np.int64), np.ascontiguousarray(e_to, dtype=np.int64),
           np.ascontiguousarray(pts, dtype=np.float64).reshape(-1)]
    ins = [a if a.size else np.zeros(1, dtype=a.dtype) for a in ins]          # (a call without any segment)
    fields = [np.ascontiguousarray(g) for g in fields]
    opt = [np.ascontiguousarray(a) for a in (w, x) if a is not None] + fields
    size, nfl = max(capacity, 1), len(fields)
    outs = [np.full(nr + GUARD, I64, dtype=np.uint64)] + [np.full(size + GUARD, p, dtype=t) for t, p in PATS]
    outs += [np.full((max(nfl, 1) if per else 1) * size + GUARD, p, dtype=t) for _, t, p, per in OUTS]
    w_per_slab = 1 if w is not None and np.ndim(w) == 3 else 0
    with ctx._temporaries(ins + opt + outs, []) as bufs:
        dn, df, dt, dp = bufs[:4]
        dw = bufs[4] if w is not None else None
        dx = bufs[4 + (w is not None)] if x is not None else None
        dg = bufs[4 + (w is not None) + (x is not None):][:nfl]
        dpc, *rec = bufs[-(len(PATS) + 1 + len(OUTS)):]
        rec, mine = rec[:len(PATS)], rec[len(PATS):]
        ptrs = [None] * len(PATS) if null_records else [b.ptr for b in rec]
        ptrs[6] = ptrs[12] = None                                            # no integrand
        gp = (nat._vp * max(nfl, 1))(*[None if m == null_g else b.ptr for m, b in enumerate(dg)])
        gd = (nat.C.c_int * max(nfl, 1))(*(g_dtype if g_dtype is not None else [nat.dtype_code(g.dtype) for g in fields]))
        gs = (nat.C.c_int * max(nfl, 1))(*[1 if g.ndim == 3 else 0 for g in fields])
        mp = [None if (null_records or name in null or (per and nfl == 0) or (not per and x is None)) else b.ptr
              for b, (name, _, _, per) in zip(mine, OUTS)]
        rc = ctx.lib.xc_contour_piece_props_dev(ctx.handle, nr, dn.ptr, df.ptr, dt.ptr, dp.ptr, ny, nx, int(periodic), int(flip), int(ncont),
                                                dw.ptr if dw is not None else None, w_per_slab, None, 0, capacity, dpc.ptr, *ptrs,
                                                nfl if nf is None else nf, nat.C.cast(gp, nat._vp), nat.C.cast(gd, nat._vp),
                                                nat.C.cast(gs, nat._vp), dx.ptr if dx is not None else None,
                                                (nat.dtype_code(x.dtype) if x is not None else 0) if x_dtype is None else x_dtype, *mp)
        pcb = dpc.download((nr + GUARD,), np.uint64)
        back = [b.download((size + GUARD,), t) for b, (t, _) in zip(rec, PATS)]
        got = [b.download(((max(nfl, 1) if per else 1) * size + GUARD,), t) for b, (_, t, _, per) in zip(mine, OUTS)]
    assert (pcb[nr:] == I64).all(), 'the guard behind piece_count was written'
    fresh = [np.full(size + GUARD, p, dtype=t) for t, p in PATS]
    npiece = int(pcb[:nr].sum()) if rc == 0 else 0
    for name, b, fr in zip(NAMES, back, fresh):
        assert b[npiece:].tobytes() == fr[npiece:].tobytes(), '%s was written behind the %d pieces' % (name, npiece)
    props = {}
    for (name, t, p, per), b in zip(OUTS, got):
        ncol = max(nfl, 1) if per else 1
        assert (b[ncol * size:] == np.array(p, dtype=t)).all(), 'the guard behind %s was written' % name
        cols = b[:ncol * size].reshape(ncol, size)
        used = npiece if (per and nfl) or (not per and x is not None) else 0
        assert (cols[:, used:] == np.array(p, dtype=t)).all(), '%s was written behind the %d pieces of a column' % (name, used)
        props[name] = cols[:nfl if per else 1, :used]
    if rc != 0:
        assert all(b.tobytes() == fr.tobytes() for b, fr in zip(back, fresh)), 'a record array was written without XC_OK'
    return rc, pcb[:nr].astype(np.int64), [b[:npiece] for b in back], props


def results(ctx, rec, ny, nx, periodic, flip, ncont, cap=None, **kw):
    """-> (per range the table (TR.DTYPE) sorted by first_edge, per range the props dict of cpprops_ref in the same rows, the groups)"""
    try:
        if cap is not None:
            ctx.set_cpiece_workspace(cap)
        rc, pc, cols, pr = call(ctx, *rec[:4], ny, nx, periodic, flip, ncont, **kw)
        groups = ctx.last_cpprops_profile()['groups']
    finally:
        if cap is not None:
            ctx.set_cpiece_workspace(DEFAULT_CAP)
    assert rc == 0, 'xc_contour_piece_props_dev returned %d' % rc
    has_x = kw.get('x') is not None
    tabs, props, p0 = [], [], 0
    for n in pc:
        n = int(n)
        t = np.empty(n, dtype=TR.DTYPE)
        for name, col in zip(NAMES, cols):
            t[name] = col[p0:p0 + n] if name not in ('sum_wf', 'net_wf') else np.nan
        par = t['parent'].copy()
        order = np.argsort(t['first_edge'], kind='stable')
        where = np.empty(n, dtype=np.int64)
        where[order] = np.arange(n)
        t['parent'] = np.where(par >= 0, where[np.clip(par - p0, 0, max(n - 1, 0))], -1) if n else par
        tabs.append(t[order])
        nfl = len(kw.get('fields', ()))
        d = {k: (pr[name][:, p0:p0 + n].T[order] if nfl and n else np.empty((n, nfl))) for k, name in (('net', 'net_g'), ('gross', 'sum_g'))}
        for k in ('x_min', 'x_max', 'at_min', 'at_max'):
            d[k] = pr[k][0, p0:p0 + n][order] if has_x else None
        props.append(d)
        p0 += n
    return tabs, props, groups


def check(ctx, rec, ny, nx, periodic, flip, ncont, what='', cap=None, w=None, fields=(), x=None, tops=None):
    tabs, props, _ = results(ctx, rec, ny, nx, periodic, flip, ncont, cap=cap, w=w, fields=fields, x=x)
    ref, rprops = QR.piece_props(*rec[:4], ny, nx, periodic, flip=flip, ncont=ncont, w=w, fields=fields, x=x, tops=tops)
    assert len(tabs) == len(ref)
    for r, (g, t, p, q) in enumerate(zip(tabs, ref, props, rprops)):
        where = '%s (periodic %d, flip %d) range %d' % (what, periodic, flip, r)
        assert TR.differences(g, t) == [], where
        assert QR.differences(p, q) == [], where
    # K19's columns are what K19's entry writes on the same records
    k19, _ = K19.tables(ctx, rec, ny, nx, periodic, flip, ncont, w=w)
    for g, t in zip(tabs, k19):
        assert g.tobytes() == t.tobytes()
    return tabs, props


def same(a, b):
    return len(a) == len(b) and all(QR.differences(u, v) == [] for u, v in zip(a, b))


def orders(rec):
    """the records in three storage orders: two shuffles and every range reversed"""
    return (shuffled(rec, 7), shuffled(rec, 8), stored(rec, [np.arange(int(c))[::-1] for c in rec[0].ravel()]))


# ------------------------------------------------------------------ the hand-built planes
@pytest.mark.parametrize('name, q, periodic', PLANES, ids=[p[0] for p in PLANES])
def test_every_hand_built_plane_in_three_storage_orders_under_two_caps(ctx, name, q, periodic):
    ny, nx = q.shape
    rng = np.random.default_rng(ny * nx)
    w, fields, x = scaled(rng, (ny, nx)), QR.field_set(rng, 3, 1, ny, nx, scaled), QR.integer_x(rng, 1, ny, nx)
    first = {}
    for flip in (0, 1):
        for k, rec in enumerate(orders(trace(q, periodic))):
            for cap in (None, 1) if k == 0 else (None,):
                (t,), (p,) = check(ctx, rec, ny, nx, periodic, flip, 1, name, cap=cap, w=w, fields=fields, x=x)
                assert QR.differences(p, first.setdefault(flip, p)) == [], 'the storage order or the cap shows'
        if t['closed'].any():
            assert np.isfinite(p['net'][t['closed']]).all() and (p['at_min'][t['closed'] & (t['n_net'] > 0)] >= 0).all()
        if name in ('chain 13', 'chain 83', 'seam'):
            assert t['depth'].max() >= 2
        if name in ('seam, plain', 'open above', 'open beside NaN', 'open beside NaN, enclosed'):
            assert (~t['closed']).any() and np.isnan(p['net'][~t['closed']]).all() and (p['at_max'][~t['closed']] == -1).all()
    assert LR.scan_geometry(ny)[1] == {600: 32, 83: 6}.get(ny, 1)            # the row-chunk regimes these planes run in


# ------------------------------------------------------------------ groups, slabs, weights, every field count
@pytest.mark.parametrize('nf', [0, 1, 3, 4, 5, 8])
@pytest.mark.parametrize('periodic', [0, 1], ids=['plain', 'ring'])
def test_twelve_ranges_in_one_group_and_in_many_at_every_field_count(ctx, periodic, nf):
    q, rec, ny, nx = K19.noise_case(periodic)
    rng = np.random.default_rng(42 + nf)
    fields = QR.field_set(rng, nf, 3, ny, nx, scaled)
    w = (None, scaled(rng, (ny, nx)), scaled(rng, (3, ny, nx)))[(nf + periodic) % 3]
    x = None if nf in (1, 5) else QR.integer_x(rng, 3, ny, nx).astype(np.float32 if nf == 4 else np.float64)   # x NULL with nf > 0; nf 0 with x
    for flip in (0, 1):
        tabs, props = check(ctx, rec, ny, nx, periodic, flip, 4, 'noise', w=w, fields=fields, x=x)
        for cap, least in ((4 * 2 * ny * nx * 4, 3), (1, 4)):                 # four ranges per group at most; one range per group
            t2, p2, groups = results(ctx, rec, ny, nx, periodic, flip, 4, cap=cap, w=w, fields=fields, x=x)
            assert groups >= least and K19.same(t2, tabs) and same(p2, props), 'the groups show'
    assert max(int(t['depth'].max()) for t in tabs if t.size) >= 1 and any((~t['closed']).any() for t in tabs)
    assert LR.scan_geometry(ny) == (16, 2)
    if x is not None:                                                        # integer values: some ring holds its extremum more than once
        sl = [np.asarray(x[r // 4], dtype=np.float64) for r in range(12)]
        _, masks = TR.piece_tree(*rec[:4], ny, nx, periodic, flip=1, ncont=4, return_masks=True)
        labs = [LR.labels_of_masks(ms, (ny, nx)) for ms in masks]
        assert any(p['x_min'][k] != 0 and ((lab == k) & (xs == p['x_min'][k])).sum() > 1 for lab, xs, p, t in zip(labs, sl, props, tabs) for k in np.flatnonzero(t['closed']))


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
    rng = np.random.default_rng(ny + nx)
    w, fields, x = scaled(rng, (1, ny, nx)), QR.field_set(rng, 5, 1, ny, nx, scaled), QR.integer_x(rng, 1, ny, nx)
    deep = 0
    for periodic in (0, 1):
        rec = shuffled(trace(q, periodic, lv), 11)
        for flip in (0, 1):
            tabs, props = check(ctx, rec, ny, nx, periodic, flip, 2, 'geometry', w=w, fields=fields, x=x)
            deep = max(deep, max(int(t['depth'].max()) for t in tabs if t.size))
    assert deep >= 1 or ny == 6


def test_one_edge_row(ctx):
    rng = np.random.default_rng(2)
    fields, x = QR.field_set(rng, 2, 1, 2, 9, scaled), QR.integer_x(rng, 1, 2, 9)
    q = np.zeros((2, 9))
    q[1, 3:6] = 1.0                                                          # ones on the last row: an open piece on a plain plane
    for periodic in (0, 1):
        for flip in (0, 1):
            (t,), (p,) = check(ctx, shuffled(trace(q, periodic), 3), 2, 9, periodic, flip, 1, 'ny 2', fields=fields, x=x)
            assert t.size == 1 and not t['closed'][0] and np.isnan(p['gross']).all() and p['at_min'][0] == -1
    q = np.zeros((2, 9))
    q[1] = 1.0                                                               # a ring that goes round, one crossing per column
    for flip in (0, 1):
        (t,), (p,) = check(ctx, shuffled(trace(q, 1), 3), 2, 9, 1, flip, 1, 'ny 2, a ring round', fields=fields, x=x)
        assert t['closed'][0] and t['winding'][0] != 0 and p['at_min'][0] // 9 == (0 if flip else 1)


def test_ranges_without_segments_wherever_they_lie_and_a_call_without_any(ctx):
    ny, nx = 24, 31
    q = np.stack([CS.smooth_noise(ny, nx, 40 + s) for s in range(2)])
    lv = np.array([-99.0, -0.3, 50.0, 60.0, 0.4, 99.0])                       # empty ranges in front, between and behind
    rec = shuffled(trace(q, 1, lv), 5)
    assert (rec[0].reshape(2, 6) > 0).tolist() == [[False, True, False, False, True, False]] * 2
    rng = np.random.default_rng(5)
    fields, x = QR.field_set(rng, 4, 2, ny, nx, scaled), QR.integer_x(rng, 2, ny, nx)
    for cap in (None, 1):
        tabs, props = check(ctx, rec, ny, nx, 1, 0, 6, 'empty ranges', cap=cap, fields=fields, x=x)
        assert all(tabs[r].size == 0 for r in (0, 2, 3, 5, 6, 8, 9, 11)) and all(tabs[r].size for r in (1, 4, 7, 10))
    none = (np.zeros(3, dtype=np.uint64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros((0, 4)))
    for capacity, null in ((4, False), (0, True)):
        rc, pc, cols, pr = call(ctx, *none, ny, nx, 0, 1, 3, capacity=capacity, null_records=null, fields=[f[:1] if f.ndim == 3 else f for f in fields],
                                x=x[:1])
        assert rc == 0 and pc.tolist() == [0, 0, 0] and pr['net_g'].size == 0


# ------------------------------------------------------------------ values that are not finite, zeros, denormals, signed zeros
def test_a_nan_term_is_skipped_and_an_inf_makes_one_field_nan_in_the_ring_and_its_ancestors(ctx):
    q = np.zeros((16, 20))
    q[1:15, 1:19] = 1.0                                                      # a block (depth 0) ...
    q[3:13, 2:9] = 0.0                                                       # ... a hole (depth 1) with an island (depth 2) in it
    q[6:9, 4:7] = 1.0
    q[3:13, 11:18] = 0.0                                                     # ... and a second hole: the first one's sibling
    ny, nx = q.shape
    rec = shuffled(trace(q, 0), 21)
    (t,), (ms,) = TR.piece_tree(*rec[:4], ny, nx, 0, return_masks=True)
    deep = int(np.flatnonzero(t['depth'] == 2)[0])
    par = int(t['parent'][deep]); top = int(t['parent'][par])
    sib = int(np.flatnonzero((t['depth'] == 1) & (np.arange(t.size) != par))[0])
    assert t.size == 4 and top >= 0 and t['parent'][top] == -1 and t['parent'][sib] == top
    rng = np.random.default_rng(3)
    fields = QR.field_set(rng, 3, 1, ny, nx, scaled)
    fields[1] = fields[1].copy(); fields[2] = fields[2].copy()
    fields[1][7, 5] = np.inf                                                 # inside the island (field 1 is a shared float32 plane)
    fields[2][0, 4, 12] = np.nan                                             # inside the sibling
    fields[2][0, 5, 12], fields[2][0, 6, 12] = 0.0, 5e-324                   # a zero and a denormal add nothing
    x = QR.integer_x(rng, 1, ny, nx)
    x[0][ms[par] & ~ms[deep]] = np.nan                                       # the hole's own nodes: all NaN
    x[0, 1, 1], x[0, 1, 2] = 0.0, -0.0                                       # the block's net nodes: -0.0 sits behind +0.0
    x[0][(ms[top] & ~ms[par] & ~ms[sib]) & (x[0] < 0)] = 7.0
    for flip in (0, 1):
        (g,), (p,) = check(ctx, rec, ny, nx, 0, flip, 1, 'not finite', fields=fields, x=x)
        assert np.isnan(p['net'][deep, 1]) and np.isnan(p['gross'][[deep, par, top], 1]).all()
        assert np.isfinite(p['net'][[par, top, sib], 1]).all() and np.isfinite(p['gross'][sib, 1])
        assert np.isfinite(p['net'][:, [0, 2]]).all() and np.isfinite(p['gross'][:, [0, 2]]).all()
        assert np.isnan(p['x_min'][par]) and p['at_min'][par] == -1 and p['at_max'][par] == -1
        assert p['x_min'][top] == 0 and np.signbit(p['x_min'][top]) and p['at_min'][top] == nx + 2


# ------------------------------------------------------------------ the capacity protocol and the refusals
def test_the_capacity_protocol_and_the_refusals(ctx):
    q, rec, ny, nx = K19.noise_case(0)
    npiece = [t.size for t in TR.PR.piece_interiors(*rec, ny, nx, 0, ncont=4)]
    rng = np.random.default_rng(9)
    fields, x = QR.field_set(rng, 3, 3, ny, nx, scaled), QR.integer_x(rng, 3, ny, nx)
    kw = dict(fields=fields, x=x)
    for cap in (None, 1):
        try:
            if cap is not None:
                ctx.set_cpiece_workspace(cap)
            rc, pc, _, _ = call(ctx, *rec, ny, nx, 0, 0, 4, capacity=0, null_records=True, **kw)
            assert rc == 1 and pc.tolist() == npiece, 'count only'
            rc, pc, _, pr = call(ctx, *rec, ny, nx, 0, 0, 4, capacity=sum(npiece) - 1, **kw)
            assert rc == 1 and pc.tolist() == npiece and pr['net_g'].size == 0, 'one record short'
            rc, pc, cols, pr = call(ctx, *rec, ny, nx, 0, 0, 4, capacity=sum(npiece), **kw)
            assert rc == 0 and pc.tolist() == npiece and cols[7].size == sum(npiece) and pr['sum_g'].shape == (3, sum(npiece)), 'an exact fit'
        finally:
            ctx.set_cpiece_workspace(DEFAULT_CAP)
    refusals = [dict(nf=-1), dict(nf=9), dict(null_g=1), dict(g_dtype=[0, 7, 1]), dict(x_dtype=2), dict(null=('sum_g',)), dict(null=('net_g',)),
                dict(null=('at_min',)), dict(null=('x_max',))]
    for r in refusals:
        rc, _, _, pr = call(ctx, *rec, ny, nx, 0, 0, 4, **kw, **r)
        assert rc == nat.XC_EBADARG and all(v.size == 0 for v in pr.values()), r
    for a_ny, a_nx, periodic, flip, ncont in ((ny, nx, 0, 2, 4), (ny, nx, 0, 0, 5), (ny, 2, 1, 0, 4)):   # K19's refusals
        rc, _, _, pr = call(ctx, *rec, a_ny, a_nx, periodic, flip, ncont, **(kw if (a_ny, a_nx) == (ny, nx) else {}))
        assert rc == nat.XC_EBADARG, (a_ny, a_nx, periodic, flip, ncont)


def test_k13_finds_a_clean_table_afterwards(ctx):
    ny, nx = 40, 65
    q = np.random.default_rng(93).integers(-3, 4, (1, ny, nx)).astype(np.float64)
    rec = shuffled(trace(q, 0, (0.0,)), 94)
    rng = np.random.default_rng(95)
    fields = QR.field_set(rng, 8, 1, ny, nx, scaled)
    tabs, props = check(ctx, rec, ny, nx, 0, 0, 1, 'integer noise', fields=fields, x=q)
    assert tabs[0]['depth'].max() >= 1
    y, xs = np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64)
    k13 = k13_tables(ctx, *rec, ny, nx, y, xs)
    ref13 = RR.pieces(*rec, ny, nx, y, xs)
    assert all(np.array_equal(g[k], t[0][k]) for g, t in zip(k13, ref13) for k in RR.INT_FIELDS)
    again, props2 = check(ctx, rec, ny, nx, 0, 0, 1, 'the call after K13', fields=fields, x=q)
    assert K19.same(again, tabs) and same(props2, props)
