"""xc_contour_piece_interiors_dev (K18), the C entry on host records, against cpinside_ref.piece_interiors: the integer fields equal,
sum_w and sum_wf equal to the header's rule BIT FOR BIT.  The records are hand-built: the restatements of K12 (contour_join_ref,
contour_join_periodic_ref) trace planes the test draws -- rings of a chosen number of segments, noise with hundreds of pieces, rings that
go round either way -- and the test then stores every range in an order of its choosing.  Weights and integrands have exponents in
[-20, 20], so every term lies wholly inside its 160-bit window: here the rule is plain math.fsum (test_cpinside_host.py shows it).
Everything else about the sums -- ties, the window's bottom and floor, bounds far from the terms, non-finite values, windows per slab --
is in test_gpu_cinside_sums.py, for K17 and K18 alike.  test_cpinside_host.py shows on the CPU what the restatement computes.
Every call hands the entry output arrays filled with a pattern and followed by guard elements: on XC_OK the records are written and every
guard intact, on 1 or a refusal nothing but piece_count is touched."""
import functools

import numpy as np
import pytest

import contour_join_periodic_ref as JP
import contour_join_ref as JR
import cpiece_records_ref as RR
import cpinside_ref as PR
from test_gpu_cpiece_records import run_records as k13_tables
from xcontour_amd import _native as nat

pytestmark = pytest.mark.gpu

DEFAULT_CAP = 1 << 30
GUARD = 16
PATS = ((np.int64, 0x5a5a5a5a5a5a5a5a), (np.int64, 0x5a5a5a5a5a5a5a5a), (np.int32, 0x5a5a5a5a), (np.int32, 0x5a5a5a5a),
        (np.int64, 0x5a5a5a5a5a5a5a5a), (np.float64, -1.2345e300), (np.float64, -1.2345e300))
NAMES = ('first_edge', 'nseg', 'closed', 'winding', 'n_in', 'sum_w', 'sum_wf')


def call(ctx, count, e_from, e_to, pts, ny, nx, periodic, flip, ncont, w=None, f=None, capacity=None, null_records=False, null_inputs=False):
    """one call -> (rc, piece_count, the seven columns as written (None where nothing may be), untouched); the guards are checked.
    null_inputs: e_from, e_to and pts are handed over as NULL (a call without any segment)"""
    count = np.ascontiguousarray(count, dtype=np.uint64).ravel()
    total, nr = int(count.sum()), count.size
    capacity = total if capacity is None else int(capacity)
    ins = [count, np.ascontiguousarray(e_from, dtype=np.int64), np.ascontiguousarray(e_to, dtype=np.int64),
           np.ascontiguousarray(pts, dtype=np.float64).reshape(-1)]
    assert ins[1].size == ins[2].size == total and ins[3].size == 4 * total
    opt = [np.ascontiguousarray(a) for a in (w, f) if a is not None]
    size = max(capacity, 1)
    outs = [np.full(nr + GUARD, 0x5a5a5a5a5a5a5a5a, dtype=np.uint64)] + [np.full(size + GUARD, p, dtype=t) for t, p in PATS]
    w_per_slab = 1 if w is not None and np.ndim(w) == 3 else 0
    with ctx._temporaries(ins + opt + outs, []) as bufs:
        dn, df, dt, dp = bufs[:4]
        dw = bufs[4] if w is not None else None
        dfi = bufs[4 + (w is not None)] if f is not None else None
        dpc, *rec = bufs[-8:]
        ptrs = [None] * 7 if null_records else [b.ptr for b in rec]
        if f is None:
            ptrs[6] = None
        recs = [None] * 3 if null_inputs else [df.ptr, dt.ptr, dp.ptr]
        rc = ctx.lib.xc_contour_piece_interiors_dev(ctx.handle, nr, dn.ptr, *recs, ny, nx, int(periodic), int(flip), int(ncont),
                                                    dw.ptr if dw is not None else None, w_per_slab, dfi.ptr if dfi is not None else None,
                                                    nat.dtype_code(f.dtype) if f is not None else 0, capacity, dpc.ptr, *ptrs)
        pcb = dpc.download((nr + GUARD,), np.uint64)
        back = [b.download((size + GUARD,), t) for b, (t, _) in zip(rec, PATS)]
    assert (pcb[nr:] == 0x5a5a5a5a5a5a5a5a).all(), 'the guard behind piece_count was written'
    fresh = [np.full(size + GUARD, p, dtype=t) for t, p in PATS]
    npiece = int(pcb[:nr].sum()) if rc == 0 else 0
    for name, b, fr in zip(NAMES, back, fresh):
        assert b[npiece:].tobytes() == fr[npiece:].tobytes(), '%s was written behind the %d pieces' % (name, npiece)
    untouched = all(b.tobytes() == fr.tobytes() for b, fr in zip(back, fresh))
    if f is None:
        assert back[6].tobytes() == fresh[6].tobytes(), 'sum_wf was written without f'
    return rc, pcb[:nr].astype(np.int64), [b[:npiece] for b in back], untouched


def tables(ctx, rec, ny, nx, periodic, flip, ncont, cap=None, **kw):
    """-> per range the table (PR.DTYPE) sorted by first_edge"""
    try:
        if cap is not None:
            ctx.set_cpiece_workspace(cap)
        rc, pc, cols, _ = call(ctx, *rec[:4], ny, nx, periodic, flip, ncont, **kw)
    finally:
        if cap is not None:
            ctx.set_cpiece_workspace(DEFAULT_CAP)
    assert rc == 0, 'xc_contour_piece_interiors_dev returned %d' % rc
    out, p0 = [], 0
    for n in pc:
        t = np.empty(int(n), dtype=PR.DTYPE)
        for name, col in zip(NAMES, cols):
            t[name] = col[p0:p0 + int(n)] if (name != 'sum_wf' or kw.get('f') is not None) else np.nan
        out.append(t[np.argsort(t['first_edge'], kind='stable')])
        p0 += int(n)
    return out


def check(ctx, rec, ny, nx, periodic, flip, ncont, what='', cap=None, w=None, f=None):
    got = tables(ctx, rec, ny, nx, periodic, flip, ncont, cap=cap, w=w, f=f)
    ref = PR.piece_interiors(*rec[:4], ny, nx, periodic, flip=flip, ncont=ncont, w=w, f=f)
    assert len(got) == len(ref)
    for r, (g, t) in enumerate(zip(got, ref)):
        bad = PR.differences(g, t)
        assert bad == [], '%s (periodic %d, flip %d) range %d: %r differ' % (what, periodic, flip, r, bad)
    return got


def same(a, b):
    return len(a) == len(b) and all(PR.differences(u, v) == [] for u, v in zip(a, b))


def scaled(rng, shape, dtype=np.float64):
    """signed values with full mantissas and exponents in [-20, 20]"""
    v = np.ldexp(rng.uniform(1.0, 2.0, shape), rng.integers(-20, 20, shape)) * rng.choice([-1.0, 1.0], shape)
    return v.astype(dtype)


def trace(q, periodic, levels=(0.5,)):
    q = np.asarray(q, dtype=np.float64)
    q = q[None] if q.ndim == 2 else q
    return (JP if periodic else JR).stack_records(q, np.asarray(levels, dtype=np.float64))


def stored(rec, orders):
    """the records with range r stored in the order orders[r] (positions -> indices inside the range)"""
    cnt, ef, et, pts = rec
    idx, s0 = [], 0
    for c, o in zip(cnt.ravel().astype(np.int64), orders):
        idx.append(s0 + np.asarray(o, dtype=np.int64))
        s0 += int(c)
    idx = np.concatenate(idx)
    return cnt.ravel(), ef[idx], et[idx], pts[idx]


def shuffled(rec, seed):
    rng = np.random.default_rng(seed)
    return stored(rec, [rng.permutation(int(c)) for c in rec[0].ravel()])


# ------------------------------------------------------------------ rings of 4 to 4097 segments
def comb(ny, nx, heights):
    """rows >= heights[c] of column c are above the level 0.5: on a ring one contour round the plane of nx + sum |h[c+1] - h[c]|
    segments (the last difference round the seam)"""
    q = np.zeros((ny, nx))
    for c, h in enumerate(heights):
        q[h:, c] = 1.0
    return q


def block(ny, nx, h, w):
    """an h x w block of ones: one ring of 2 (h + w) segments"""
    q = np.zeros((ny, nx))
    q[2:2 + h, 1:1 + w] = 1.0
    return q


@functools.lru_cache(maxsize=None)
def ring_planes():
    """name -> (q (70, 65), periodic, the segments of its one ring)"""
    ny, nx = 70, 65
    return {'blob 4': (block(ny, nx, 1, 1), 0, 4), 'block 64': (block(ny, nx, 15, 17), 0, 64), 'block 66': (block(ny, nx, 16, 17), 0, 66),
            'block 256': (block(ny, nx, 66, 62), 0, 256), 'round 65': (comb(ny, nx, [30] * nx), 1, 65),
            'round 257': (comb(ny, nx, [30, 33] * 32 + [30]), 1, 257), 'round 4097': (comb(ny, nx, [2, 65] * 32 + [2]), 1, 4097),
            'hole 4': (1.0 - block(ny, nx, 1, 1), 0, 4), 'round the other way': (1.0 - comb(ny, nx, [30, 33, 32] * 21 + [30, 31]), 1, None)}


@pytest.mark.parametrize('cap', [None, 1], ids=['default cap', 'one range per group'])
@pytest.mark.parametrize('periodic', [0, 1], ids=['plain', 'ring'])
def test_rings_of_4_to_4097_segments_in_four_storage_orders(ctx, periodic, cap):
    ny, nx = 70, 65
    rng = np.random.default_rng(81)
    w, f = scaled(rng, (ny, nx)), scaled(rng, (1, ny, nx))
    planes = [(k, v) for k, v in ring_planes().items() if v[1] == periodic]
    recs = [trace(q, periodic) for _, (q, _, _) in planes]
    for (name, (_, _, n)), rec in zip(planes, recs):
        assert n is None or int(rec[0].sum()) == n, name
    CNT, EF, ET, PT = [], [], [], []
    for rec in recs:
        n = int(rec[0].sum())
        for o in RR.storage_orders(n, rng).values():
            c, a, b, p = stored(rec, [o])
            CNT.append(c); EF.append(a); ET.append(b); PT.append(p)
    rec = (np.concatenate(CNT), np.concatenate(EF), np.concatenate(ET), np.concatenate(PT))
    for flip in (0, 1):
        got = check(ctx, rec, ny, nx, periodic, flip, rec[0].size, 'rings', cap=cap, w=w, f=f)
        assert all(t.size == 1 and t['closed'][0] for t in got)
        for k in range(0, len(got), 4):
            assert all(same([got[k]], [got[k + j]]) for j in range(1, 4)), 'the storage order shows'
    if periodic:
        assert sorted({int(t['winding'][0]) for t in got}) == [-1, 1]
    else:
        assert sorted({int(t['n_in'][0]) for t in got}) == [1, 15 * 17, 16 * 17, 66 * 62]


# ------------------------------------------------------------------ hundreds of pieces, every width, three caps
def noise(ny, nx, nslab, seed, nan=True):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((nslab, ny, nx)) + np.linspace(-2.0, 2.0, ny)[None, :, None]
    if nan:
        q[0, ny // 2:ny // 2 + 2, nx // 3:nx // 3 + 2] = np.nan
        q[-1, ny - 2, 0] = np.nan
        q[-1, 0, nx - 1] = np.nan
    return q


SHAPES = [(63, 63), (64, 64), (65, 65), (130, 70), (7, 130)]


@pytest.mark.parametrize('periodic', [0, 1], ids=['plain', 'ring'])
@pytest.mark.parametrize('shape', SHAPES, ids=['%dx%d' % s for s in SHAPES])
def test_noise_with_nan_cells_every_weight_and_integrand_under_three_caps(ctx, shape, periodic):
    """two slabs, three levels (one on a node's value): hundreds of pieces per range -- rings in rings, open pieces beside the NaN cells
    and the edges, on a ring the contours that go round -- in a shuffled storage order; w shared, per slab and NULL; f float32, float64
    and NULL; all ranges in one group, one range per group, two per group"""
    ny, nx = shape
    q = noise(ny, nx, 2, 90 + ny + nx)
    lv = np.sort(np.array([-0.7, q[1, 3, 3], 0.8]))
    rec = shuffled(trace(q, periodic, lv), 91)
    rng = np.random.default_rng(92 + nx)
    w2, w3 = scaled(rng, (ny, nx)), scaled(rng, (2, ny, nx))
    f32, f64 = scaled(rng, (2, ny, nx), np.float32), scaled(rng, (2, ny, nx))
    variants = [dict(w=w2, f=f64), dict(w=w3, f=f32), dict(w=None, f=None), dict(w=None, f=f64)]
    two = 2 * (2 * ny * nx) * 4
    for k, flip in enumerate((0, 1, 1, 0)):
        v = variants[(k + periodic) % 4]
        got = check(ctx, rec, ny, nx, periodic, flip, 3, 'noise %r' % (shape,), **v)
        assert same(tables(ctx, rec, ny, nx, periodic, flip, 3, cap=1, **v), got), 'one range per group against one group'
        assert same(tables(ctx, rec, ny, nx, periodic, flip, 3, cap=two, **v), got), 'two ranges per group against one group'
        if v['w'] is None:
            for t in got:
                assert np.array_equal(t['sum_w'][t['closed']], t['n_in'][t['closed']].astype(np.float64))
    if ny >= 63:
        assert max(t.size for t in got) >= 100 and any((~t['closed']).any() for t in got)
        assert any((t['closed'] & (t['n_in'] > 20)).any() for t in got)
        if periodic:
            assert any((t['winding'] != 0).any() for t in got)


def test_several_hundred_pieces_in_one_range_and_empty_ranges_around_it(ctx):
    ny, nx = 40, 65
    q = np.random.default_rng(93).integers(-3, 4, (1, ny, nx)).astype(np.float64)
    cnt, ef, et, pts = shuffled(trace(q, 1, (1.0,)), 94)
    rec = (np.array([0, cnt[0], 0, cnt[0], 0], dtype=np.uint64), np.concatenate([ef, ef[::-1]]), np.concatenate([et, et[::-1]]),
           np.concatenate([pts, pts[::-1]]))
    rng = np.random.default_rng(95)
    w, f = scaled(rng, (ny, nx)), scaled(rng, (1, ny, nx))
    runs = [check(ctx, rec, ny, nx, 1, 0, 5, 'many pieces', cap=cap, w=w, f=f) for cap in (None, 1, 2 * (2 * ny * nx) * 4)]
    assert same(runs[1], runs[0]) and same(runs[2], runs[0])
    assert runs[0][1].size >= 300 and runs[0][0].size == 0 and same([runs[0][1]], [runs[0][3]])


def test_windings_minus_one_zero_and_plus_one(ctx):
    ny, nx = 12, 9
    q = np.zeros((2, ny, nx))
    q[0, 6:] = 1.0
    q[0, 2:6, 3] = 1.0
    q[0, 2, 3:6] = 1.0                                                       # the S-fold of the host test
    q[0, 9, 1] = 0.0                                                         # a hole below the ring
    q[1] = 1.0 - q[0]                                                        # the same contours the other way round
    rec = shuffled(trace(q, 1), 96)
    for flip in (0, 1):
        got = check(ctx, rec, ny, nx, 1, flip, 1, 'windings')
        assert sorted(got[0]['winding'].tolist() + got[1]['winding'].tolist()) == [-1, 0, 0, 1]
        for t, qs in zip(got, q):
            main = t[t['winding'] != 0][0]
            below = int((q[0] > 0.5).sum()) + 1                                # the nodes below the ring, the hole's among them
            assert main['n_in'] == (ny * nx - below if flip else below)
            assert t[t['winding'] == 0]['n_in'].tolist() == [1]                # flip does not touch a ring of winding 0


# ------------------------------------------------------------------ non-finite terms
def test_a_nan_term_is_skipped_and_an_infinite_one_poisons_that_sum_of_that_piece_alone(ctx):
    ny, nx = 12, 14
    q = np.zeros((ny, nx))
    q[2:5, 2:5] = 1.0                                                        # piece A: 9 nodes
    q[7:10, 2:5] = 1.0                                                       # piece B: 9 nodes, the same columns
    q[2:5, 8:11] = 1.0                                                       # piece C
    rec = shuffled(trace(q[None], 0), 97)
    rng = np.random.default_rng(98)
    w, f = scaled(rng, (ny, nx)), scaled(rng, (1, ny, nx))
    w[3, 3] = np.inf                                                         # A: sum_w and sum_wf (inf * finite) are NaN
    f[0, 8, 3] = -np.inf                                                     # B: sum_wf alone
    w[3, 9] = np.nan                                                         # C: the term is skipped in both sums
    w[0, 0] = np.inf                                                         # outside every piece
    (t,) = check(ctx, rec, ny, nx, 0, 0, 1, 'non-finite', w=w, f=f)
    assert t['n_in'].tolist() == [9, 9, 9]
    a, c, b = t[0], t[1], t[2]                                               # first_edge order: A, C (rows 2..), B
    assert np.isnan(a['sum_w']) and np.isnan(a['sum_wf'])
    assert np.isfinite(b['sum_w']) and np.isnan(b['sum_wf'])
    assert np.isfinite(c['sum_w']) and np.isfinite(c['sum_wf'])


# ------------------------------------------------------------------ the capacity protocol and the refusals
def test_the_capacity_protocol(ctx):
    ny, nx = 40, 65
    q = np.random.default_rng(93).integers(-3, 4, (2, ny, nx)).astype(np.float64)
    rec = shuffled(trace(q, 0, (-1.0, 1.0)), 99)
    ref = PR.piece_interiors(*rec, ny, nx, 0, ncont=2)
    npiece = [t.size for t in ref]
    for cap in (None, 1):                                                    # the count must not depend on where a group ends
        try:
            if cap is not None:
                ctx.set_cpiece_workspace(cap)
            rc, pc, _, untouched = call(ctx, *rec, ny, nx, 0, 0, 2, capacity=0, null_records=True)
            assert rc == 1 and pc.tolist() == npiece and untouched, 'count only'
            rc, pc, _, untouched = call(ctx, *rec, ny, nx, 0, 0, 2, capacity=sum(npiece) - 1)
            assert rc == 1 and pc.tolist() == npiece and untouched, 'one record short'
            rc, pc, _, untouched = call(ctx, *rec, ny, nx, 0, 0, 2, capacity=npiece[0])
            assert rc == 1 and pc.tolist() == npiece and untouched, 'room for the first range alone'
            rc, pc, cols, _ = call(ctx, *rec, ny, nx, 0, 0, 2, capacity=sum(npiece))
            assert rc == 0 and pc.tolist() == npiece and cols[0].size == sum(npiece), 'an exact fit'
            assert sorted(cols[0][:npiece[0]].tolist()) == ref[0]['first_edge'].tolist()
        finally:
            ctx.set_cpiece_workspace(DEFAULT_CAP)


def test_bad_arguments_are_refused_and_nothing_is_written(ctx):
    ny, nx = 12, 9
    rec = trace(np.pad(np.ones((4, 3)), 4)[:ny, :nx], 0)
    for a_ny, a_nx, periodic, flip, ncont in ((ny, nx, 0, 2, 1), (ny, nx, 0, 0, 0), (ny, nx, 0, 0, 2), (1 << 16, 1 << 14, 0, 0, 1),
                                              (6, 2, 1, 0, 1)):
        rc, _, _, untouched = call(ctx, *rec, a_ny, a_nx, periodic, flip, ncont)
        assert rc == nat.XC_EBADARG and untouched, (a_ny, a_nx, periodic, flip, ncont)


@pytest.mark.parametrize('which,value', [('e_from', 2 * 40 * 65), ('e_to', -1)])
def test_an_edge_id_out_of_range_is_refused_and_the_tables_are_handed_on_clean(ctx, which, value):
    ny, nx = 40, 65
    q = np.random.default_rng(93).integers(-3, 4, (1, ny, nx)).astype(np.float64)
    rec = shuffled(trace(q, 0, (0.0,)), 94)
    bad_f, bad_t = rec[1].copy(), rec[2].copy()
    (bad_f if which == 'e_from' else bad_t)[517] = value
    rc, _, _, untouched = call(ctx, rec[0], bad_f, bad_t, rec[3], ny, nx, 0, 0, 1)
    assert rc == nat.XC_EBADARG and untouched
    # K13 on the same workspace straight afterwards, then this entry again
    y, x = np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64)
    k13 = k13_tables(ctx, *rec, ny, nx, y, x)
    ref13 = RR.pieces(*rec, ny, nx, y, x)
    assert all(np.array_equal(g[k], t[0][k]) for g, t in zip(k13, ref13) for k in RR.INT_FIELDS)
    got = check(ctx, rec, ny, nx, 0, 0, 1, 'the call after the refused one')
    assert all(np.array_equal(g[k], t[k]) for g, t in zip(got, k13) for k in RR.INT_FIELDS)
