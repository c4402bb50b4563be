"""xc_contour_interior_dev (K17), the C entry on device records, against cinside_ref: n_in and the mask equal, sum_w and sum_wf equal
to the header's rule BIT FOR BIT.  The records are K12's own (Context.contour_segments of a small field) or built by the test.  Weights
and integrands have exponents in [-20, 20], so every term of either sum lies within 2^+-40 and wholly inside its 160-bit window: here
the rule is plain math.fsum (test_cinside_host.py shows it).  Everything else about the sums -- ties, the window's bottom and floor,
bounds far from the terms, non-finite values, windows per slab -- is in test_gpu_cinside_sums.py; the cuts of the scan's launch geometry
are in test_gpu_cinside_geometry.py.  test_cinside_host.py shows on the CPU what the restatement computes.  Every call hands the entry
output arrays filled with a pattern and followed by guard elements: on XC_OK every element is written and every guard intact, on a
refusal before the first launch nothing is touched."""
import numpy as np
import pytest

import cinside_ref as IR
import cpiece_records_ref as RR
from xcontour_amd import _native as nat

pytestmark = pytest.mark.gpu

DEFAULT_CAP = 1 << 30
GUARD = 16
PAT_I64, PAT_F64, PAT_U8 = 0x5a5a5a5a5a5a5a5a, -1.2345e300, 0xa5
SELECTS = ((0, 0), (1, 0), (1, 1), (1, 2))                                   # (periodic, select)


def call(ctx, count, e_from, e_to, pts, ny, nx, periodic, select, flip, ncont, w=None, f=None, want_mask=True, w_per_slab=None,
         null_records=False):
    """one xc_contour_interior_dev call on host records -> (rc, dict(n_in, sum_w, sum_wf, mask), untouched); the guards are checked.
    null_records: e_from, e_to and pts are handed over as NULL (a call without any segment)"""
    count = np.ascontiguousarray(count, dtype=np.uint64).ravel()
    total, nr = int(count.sum()), count.size
    ins = [count, np.ascontiguousarray(e_from, dtype=np.int64), np.ascontiguousarray(e_to, dtype=np.int64),
           np.ascontiguousarray(pts, dtype=np.float64)]
    assert ins[1].size == ins[2].size == total and ins[3].size == 4 * total
    opt = [np.ascontiguousarray(a) for a in (w, f) if a is not None]
    sizes = [nr, nr, nr, nr * ny * nx]
    pats = [(np.int64, PAT_I64), (np.float64, PAT_F64), (np.float64, PAT_F64), (np.uint8, PAT_U8)]
    outs = [np.full(n + GUARD, p, dtype=t) for n, (t, p) in zip(sizes, pats)]
    if w_per_slab is None:
        w_per_slab = 1 if w is not None and np.ndim(w) == 3 else 0
    with ctx._temporaries(ins + opt + outs, []) as bufs:
        dn, df, dt, dp = bufs[:4]
        dw = bufs[4] if w is not None else None
        dfi = bufs[4 + (w is not None)] if f is not None else None
        dni, dsw, dsf, dm = bufs[-4:]
        recs = [None] * 3 if null_records else [df.ptr, dt.ptr, dp.ptr]
        rc = ctx.lib.xc_contour_interior_dev(ctx.handle, nr, dn.ptr, *recs, ny, nx, int(periodic), int(select), int(flip),
                                             int(ncont), dw.ptr if dw is not None else None, int(w_per_slab),
                                             dfi.ptr if dfi is not None else None, nat.dtype_code(f.dtype) if f is not None else 0,
                                             dni.ptr, dsw.ptr, dsf.ptr if f is not None else None, dm.ptr if want_mask else None)
        back = [b.download((n + GUARD,), t) for b, n, (t, _) in zip((dni, dsw, dsf, dm), sizes, pats)]
    fresh = [np.full(n + GUARD, p, dtype=t) for n, (t, p) in zip(sizes, pats)]
    for name, b, fr, n in zip(('n_in', 'sum_w', 'sum_wf', 'mask'), back, fresh, sizes):
        assert b[n:].tobytes() == fr[n:].tobytes(), 'the guard behind %s was written' % name
    untouched = all(b.tobytes() == fr.tobytes() for b, fr in zip(back, fresh))
    if f is None:
        assert back[2].tobytes() == fresh[2].tobytes(), 'sum_wf was written without f'
    if not want_mask:
        assert back[3].tobytes() == fresh[3].tobytes(), 'the mask was written though none was asked for'
    res = dict(n_in=back[0][:nr], sum_w=back[1][:nr], sum_wf=back[2][:nr] if f is not None else None,
               mask=back[3][:nr * ny * nx].reshape(nr, ny, nx) if want_mask else None)
    return rc, res, untouched


def run(ctx, rec, ny, nx, periodic, select, flip, ncont, cap=None, **kw):
    try:
        if cap is not None:
            ctx.set_cpiece_workspace(cap)
        rc, res, _ = call(ctx, *rec[:4], ny, nx, periodic, select, flip, ncont, **kw)
    finally:
        if cap is not None:
            ctx.set_cpiece_workspace(DEFAULT_CAP)
    assert rc == 0, 'xc_contour_interior_dev returned %d' % rc
    return res


def differences(got, ref):
    bad = []
    if not np.array_equal(got['n_in'], ref['n_in']):
        bad.append('n_in')
    if got['mask'] is not None and not np.array_equal(got['mask'], ref['mask']):
        bad.append('mask')
    for k in ('sum_w', 'sum_wf'):
        if (got[k] is None) != (ref[k] is None) or (got[k] is not None and not IR.same_bits(got[k], ref[k])):
            bad.append(k)
    return bad


def check(ctx, rec, ny, nx, periodic, select, flip, ncont, what='', cap=None, w=None, f=None, want_mask=True):
    got = run(ctx, rec, ny, nx, periodic, select, flip, ncont, cap=cap, w=w, f=f, want_mask=want_mask)
    ref = IR.interior(*rec[:4], ny, nx, periodic, select, flip=flip, ncont=ncont, w=w, f=f)
    bad = differences(got, ref)
    assert bad == [], '%s (periodic %d, select %d, flip %d): %r differ' % (what, periodic, select, flip, bad)
    return got, ref


def scaled(rng, shape, dtype=np.float64):
    """signed values with full mantissas and exponents in [-20, 20]"""
    v = np.ldexp(rng.uniform(1.0, 2.0, shape), rng.integers(-20, 20, shape)) * rng.choice([-1.0, 1.0], shape)
    return v.astype(dtype)


def field(shape, nslab, seed, nan=False):
    rng = np.random.default_rng(seed)
    ny, nx = shape
    q = rng.standard_normal((nslab, ny, nx)) + np.linspace(-1.5, 1.5, ny)[None, :, None]
    if nan:
        q[0, ny // 2, nx // 3] = np.nan
        q[-1, max(ny - 3, 0):ny - 1, 0:2] = np.nan
        q[-1, 0, nx - 1] = np.nan
    return q


def levels(q, n):
    """n ascending levels: the first below the field and the last above it (no segments), one of them a node's value"""
    if n == 1:
        return np.array([0.1])
    lv = np.linspace(-2.0, 2.0, n)
    lv[0], lv[-1] = -50.0, 50.0
    if n > 2:
        lv[n // 2] = q[0, 0, 0] if np.isfinite(q[0, 0, 0]) else lv[n // 2]
    return np.sort(lv)


SHAPES = [(2, 2), (2, 65), (3, 64), (9, 70), (33, 130), (130, 7)]


@pytest.mark.parametrize('shape', SHAPES, ids=['%dx%d' % s for s in SHAPES])
def test_k12_records_every_select_flip_weight_and_integrand(ctx, shape):
    """two slabs, three levels; both planes, the three selections, both flips; w shared, per slab and NULL; f float32, float64 and
    NULL; with and without the mask; one range per group and all ranges in one"""
    ny, nx = shape
    q = field(shape, 2, 50 + ny)
    lv = levels(q, 3)
    rng = np.random.default_rng(60 + nx)
    w2, w3 = scaled(rng, (ny, nx)), scaled(rng, (2, ny, nx))
    f32, f64 = scaled(rng, (2, ny, nx), np.float32), scaled(rng, (2, ny, nx))
    variants = [dict(w=w2, f=f64), dict(w=w3, f=f32), dict(w=None, f=None), dict(w=w2, f=None), dict(w=None, f=f64)]
    k = 0
    for periodic, select in SELECTS:
        cnt, ef, et, pts = ctx.contour_segments(q, lv, periodic=bool(periodic))
        rec = (cnt.ravel(), ef, et, pts)
        for flip in (0, 1):
            v = variants[k % len(variants)]
            k += 1
            got, ref = check(ctx, rec, ny, nx, periodic, select, flip, 3, 'k12 %r' % (shape,), **v)
            one = run(ctx, rec, ny, nx, periodic, select, flip, 3, cap=1, **v)
            assert differences(one, got) == [], 'one range per group against one group'
            bare = run(ctx, rec, ny, nx, periodic, select, flip, 3, want_mask=False, **v)
            assert differences(bare, got) == []
            if v['w'] is None:
                assert np.array_equal(got['sum_w'], got['n_in'].astype(np.float64))
            assert np.array_equal(got['n_in'], got['mask'].reshape(6, -1).sum(axis=1))
        if select == 0:
            # the threshold identity, levels on node values included
            above = q[:, None] > lv[None, :, None, None]
            assert np.array_equal(got['mask'].reshape(2, 3, ny, nx).astype(bool), ~(above ^ above[:, :, :1]))


@pytest.mark.parametrize('nlev', [1, 70])
@pytest.mark.parametrize('shape', [(9, 70), (33, 130), (130, 7)], ids=['9x70', '33x130', '130x7'])
def test_one_and_seventy_levels_on_a_field_with_nan_cells(ctx, shape, nlev):
    ny, nx = shape
    q = field(shape, 2, 70 + ny, nan=True)
    lv = levels(q, nlev)
    rng = np.random.default_rng(71)
    w, f = scaled(rng, (2, ny, nx)), scaled(rng, (2, ny, nx), np.float32)
    for periodic, select in ((0, 0), (1, 2), (1, 0)):
        cnt, ef, et, pts = ctx.contour_segments(q, lv, periodic=bool(periodic))
        rec = (cnt.ravel(), ef, et, pts)
        got, _ = check(ctx, rec, ny, nx, periodic, select, 0, nlev, 'nan cells', w=w, f=f)
        if nlev > 1:
            assert cnt[:, 0].sum() == 0 and cnt[:, -1].sum() == 0 and not got['mask'][0].any() and not got['mask'][nlev - 1].any()
            mid = 3 * (2 * ny * nx) * 4                                      # three ranges per group
            assert differences(run(ctx, rec, ny, nx, periodic, select, 0, nlev, cap=mid, w=w, f=f), got) == []
            assert differences(run(ctx, rec, ny, nx, periodic, select, 0, nlev, cap=1, w=w, f=f), got) == []


def test_a_nan_term_is_skipped_and_an_infinite_one_poisons_its_range_alone(ctx):
    ny, nx = 9, 70
    q = np.repeat(np.arange(ny, dtype=np.float64)[:, None], nx, axis=1)[None]
    lv = np.array([2.5, 6.5])                                                # inside: rows 3.. and rows 7..
    cnt, ef, et, pts = ctx.contour_segments(q, lv, periodic=True)
    rec = (cnt.ravel(), ef, et, pts)
    rng = np.random.default_rng(72)
    w, f = scaled(rng, (ny, nx)), scaled(rng, (1, ny, nx))
    w[4, 5] = np.inf                                                         # inside the first range only
    w[8, 1] = np.nan                                                         # inside both: skipped in both sums
    f[0, 7, 7] = np.nan                                                      # inside both: skipped in sum_wf only
    f[0, 5, 9] = -np.inf                                                     # the first range
    w[0, 0] = np.inf                                                         # outside both (inside both under flip)
    got, ref = check(ctx, rec, ny, nx, 1, 2, 0, 2, 'non-finite', w=w, f=f)
    assert np.isnan(got['sum_w'][0]) and np.isnan(got['sum_wf'][0]) and np.isfinite(got['sum_w'][1]) and np.isfinite(got['sum_wf'][1])
    assert got['n_in'].tolist() == [6 * nx, 2 * nx]
    got, _ = check(ctx, rec, ny, nx, 1, 2, 1, 2, 'non-finite, flipped', w=w, f=f)
    assert np.isnan(got['sum_w']).all() and np.isnan(got['sum_wf']).all()
    w[0, 0] = 0.0
    f[0, 0, 0] = np.inf                                                      # 0 * inf: a NaN term, skipped
    got, _ = check(ctx, rec, ny, nx, 1, 2, 1, 2, '0 * inf', w=w, f=f)
    assert np.isfinite(got['sum_w'][0]) and np.isfinite(got['sum_wf'][0]) and np.isnan(got['sum_w'][1]) and np.isnan(got['sum_wf'][1])


# ------------------------------------------------------------------ hand-built records
def test_an_open_piece_whose_tail_lies_on_a_vertical_edge(ctx):
    """H(0, 1) -> V(1, 3) -> V(2, 4): the start point on V(1, 3) and the tail on V(2, 4) are crossings, the head on a horizontal edge
    is none"""
    ny, nx = 4, 6
    V = lambda r, c: 2 * (r * nx + c) + 1
    H = lambda r, c: 2 * (r * nx + c)
    ef, et = RR.chain([H(0, 1), V(1, 3)], False, V(2, 4))
    pts = np.array([[0.0, 1.5, 1.5, 3.0], [1.5, 3.0, 2.5, 4.0]])
    rec = (np.array([2], dtype=np.uint64), ef, et, pts)
    expect = np.zeros((ny, nx), dtype=np.uint8)
    expect[2:, 3] = 1
    expect[3, 4] = 1
    for periodic in (0, 1):
        got, _ = check(ctx, rec, ny, nx, periodic, 0, 0, 1, 'open piece')
        assert np.array_equal(got['mask'][0], expect) and got['n_in'].tolist() == [3]
        got, _ = check(ctx, rec, ny, nx, periodic, 0, 1, 1, 'open piece, flipped')
        assert np.array_equal(got['mask'][0], 1 - expect) and got['n_in'].tolist() == [ny * nx - 3]
    got, _ = check(ctx, rec, ny, nx, 1, 2, 0, 1, 'open piece under main')     # no ring: nothing is selected
    assert not got['mask'].any()
    # stored the other way round
    rev = (rec[0], ef[::-1].copy(), et[::-1].copy(), pts[::-1].copy())
    assert np.array_equal(check(ctx, rev, ny, nx, 0, 0, 0, 1, 'reversed')[0]['mask'][0], expect)


def test_two_rings_that_share_a_column(ctx):
    """ring A meets column 2 on V(0, 2) and V(2, 2), ring B on V(3, 2) and V(5, 2); B goes round the ring of columns once (one end
    point on column nx) and is the main ring, A is an ordinary ring"""
    ny, nx = 8, 6
    V = lambda r, c: 2 * (r * nx + c) + 1
    H = lambda r, c: 2 * (r * nx + c)
    a, b = [V(0, 2), H(0, 2), V(2, 2), H(3, 1)], [V(3, 2), H(4, 2), V(5, 2), H(6, 1)]
    fa, ta = RR.chain(a, True)
    fb, tb = RR.chain(b, True)
    pts = np.zeros((8, 4))
    pts[5, 3] = float(nx)
    order = np.array([6, 1, 4, 3, 0, 7, 2, 5])
    rec = (np.array([8], dtype=np.uint64), np.concatenate([fa, fb])[order], np.concatenate([ta, tb])[order], pts[order])
    both = np.zeros((ny, nx), dtype=np.uint8)
    both[1:3, 2] = 1
    both[4:6, 2] = 1
    only_b = np.zeros((ny, nx), dtype=np.uint8)
    only_b[4:6, 2] = 1
    for periodic, select, expect in ((0, 0, both), (1, 0, both), (1, 1, only_b), (1, 2, only_b)):
        got, _ = check(ctx, rec, ny, nx, periodic, select, 0, 1, 'two rings')
        assert np.array_equal(got['mask'][0], expect)
    # two ranges of one slab and the same records in each: ncont 2, both ranges alike
    two = (np.array([8, 8], dtype=np.uint64),) + tuple(np.concatenate([r, r]) for r in rec[1:])
    got, _ = check(ctx, two, ny, nx, 1, 2, 0, 2, 'two ranges')
    assert np.array_equal(got['mask'][0], only_b) and np.array_equal(got['mask'][1], only_b)


def test_many_pieces_with_random_ids_under_three_caps(ctx):
    """450 pieces on random edge ids (rows up to ny - 1, whose vertical edges bound no node), empty ranges in front, between and
    behind"""
    ny, nx = 8, 300
    cnt, ef, et, pts, _ = RR.many_pieces(ny, nx)
    rec = (np.array([0, cnt[0], 0, cnt[0], 0], dtype=np.uint64), np.concatenate([ef, ef]), np.concatenate([et, et]), np.concatenate([pts, pts]))
    rng = np.random.default_rng(73)
    w, f = scaled(rng, (ny, nx)), scaled(rng, (1, ny, nx))
    runs = [check(ctx, rec, ny, nx, 1, 0, 0, 5, 'many pieces', cap=cap, w=w, f=f)[0] for cap in (None, 1, 2 * (2 * ny * nx) * 4)]
    assert differences(runs[1], runs[0]) == [] and differences(runs[2], runs[0]) == []
    assert not runs[0]['mask'][0].any() and runs[0]['mask'][1].any() and np.array_equal(runs[0]['mask'][1], runs[0]['mask'][3])


# ------------------------------------------------------------------ refusals
def test_bad_arguments_are_refused_and_nothing_is_written(ctx):
    ny, nx = 8, 300
    cnt, ef, et, pts, _ = RR.many_pieces(ny, nx)
    for periodic, select, flip, ncont in ((0, 1, 0, 1), (0, 2, 0, 1), (1, 3, 0, 1), (1, -1, 0, 1), (1, 0, 2, 1), (1, 0, 0, 0), (1, 0, 0, 2)):
        rc, _, untouched = call(ctx, cnt, ef, et, pts, ny, nx, periodic, select, flip, ncont)
        assert rc == nat.XC_EBADARG and untouched, (periodic, select, flip, ncont)


@pytest.mark.parametrize('which,value', [('e_from', 2 * 8 * 300), ('e_to', -1)])
def test_an_edge_id_out_of_range_is_refused_and_the_next_call_is_right(ctx, which, value):
    ny, nx = 8, 300
    cnt, ef, et, pts, _ = RR.many_pieces(ny, nx)
    bad_f, bad_t = ef.copy(), et.copy()
    (bad_f if which == 'e_from' else bad_t)[517] = value
    rc, _, _ = call(ctx, cnt, bad_f, bad_t, pts, ny, nx, 1, 2, 0, 1)
    assert rc == nat.XC_EBADARG
    check(ctx, (cnt, ef, et, pts), ny, nx, 1, 0, 0, 1, 'the call after the refused one')
