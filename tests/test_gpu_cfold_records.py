"""xc_contour_folds_dev (K24), the C entry on device records, against cfold_ref: integers equal, rows and sums BIT FOR BIT.  The
records are K12's own (Context.contour_segments) of the hand-built planes of cfold_ref.cases(): q = far ? 1 : 0 with level 0.5, so the
crossings are exactly the mask's transitions.  test_cfold_host.py shows on the CPU what the restatement computes on these planes.
Every call hands the entry output arrays filled with a pattern and followed by guard elements: the dense arrays and event_count are
always fully written, the event arrays only when the events fit, and no guard is ever touched."""
import math

import numpy as np
import pytest

import cfold_ref as FR
import cinside_ref as IR
from xcontour_amd import _native as nat

pytestmark = pytest.mark.gpu

DEFAULT_CAP = 1 << 30
GUARD = 16
PAT = {np.int32: 0x5a5a5a5a, np.int64: 0x5a5a5a5a5a5a5a5a, np.uint64: 0x5a5a5a5a5a5a5a5a, np.float64: -1.2345e300}
DENSE = (('ncross', np.int32), ('row_lo', np.float64), ('row_hi', np.float64), ('col_event', np.int32))
EVENT = (('c_west', np.int32, 1), ('c_east', np.int32, 1), ('ncol', np.int32, 1), ('ncross_max', np.int32, 1), ('ev_row_lo', np.float64, 1),
         ('ev_row_hi', np.float64, 1), ('nodes', np.int64, 2), ('area', np.float64, 2), ('mx', np.float64, 2), ('my', np.float64, 2),
         ('integral', np.float64, 2))
CASES = FR.cases()


def call(ctx, count, e_from, e_to, pts, ny, nx, periodic, select, ncont, gap, w=None, f=None, capacity=None):
    """one xc_contour_folds_dev call on host records (capacity None: a count-only call first, then one of exactly that size)
    -> (rc, result dict, events_untouched); the guards are checked"""
    count = np.ascontiguousarray(count, dtype=np.uint64).ravel()
    total, nr = int(count.sum()), count.size
    ins = [count, np.ascontiguousarray(e_from, dtype=np.int64), np.ascontiguousarray(e_to, dtype=np.int64),
           np.ascontiguousarray(pts, dtype=np.float64)]
    assert ins[1].size == ins[2].size == total and ins[3].size == 4 * total
    opt = [np.ascontiguousarray(a) for a in (w, f) if a is not None]
    wps = 1 if w is not None and np.ndim(w) == 3 else 0

    def once(cap, with_events):
        fresh = [np.full(nr * nx + GUARD, PAT[t], dtype=t) for _, t in DENSE] + [np.full(nr + GUARD, PAT[np.uint64], dtype=np.uint64)]
        if with_events:
            fresh += [np.full(max(cap, 1) * k + GUARD, PAT[t], dtype=t) for _, t, k in EVENT]
        with ctx._temporaries(ins + opt + fresh, []) as bufs:
            dn, df, dt, dp = bufs[:4]
            dw = bufs[4] if w is not None else None
            dfi = bufs[4 + (w is not None)] if f is not None else None
            outs = bufs[4 + len(opt):]
            ev = [b.ptr for b in outs[5:]] if with_events else [None] * len(EVENT)
            if f is None:
                ev[-1] = None
            recs = [df.ptr, dt.ptr, dp.ptr] if total else [None] * 3
            rc = ctx.lib.xc_contour_folds_dev(ctx.handle, nr, dn.ptr, *recs, ny, nx, int(periodic), int(select), int(ncont),
                                              dw.ptr if dw is not None else None, wps, dfi.ptr if dfi is not None else None,
                                              nat.dtype_code(f.dtype) if f is not None else 0, int(gap), *[b.ptr for b in outs[:4]],
                                              int(cap), outs[4].ptr, *ev)
            back = [b.download(a.shape, a.dtype) for b, a in zip(outs, fresh)]
        return rc, back, fresh

    if capacity is None:
        rc, back, fresh = once(0, False)
        assert rc in (0, 1), 'the count-only call returned %d' % rc
        capacity = int(back[4][:nr].sum())
        assert (rc == 1) == (capacity > 0)
        first = back
    else:
        first = None
    rc, back, fresh = once(capacity, True)
    sizes = [nr * nx] * 4 + [nr] + [max(capacity, 1) * k for _, _, k in EVENT]
    names = [d[0] for d in DENSE] + ['event_count'] + [e[0] for e in EVENT]
    for name, b, fr, n in zip(names, back, fresh, sizes):
        assert b[n:].tobytes() == fr[n:].tobytes(), 'the guard behind %s was written' % name
    if f is None:
        assert back[-1].tobytes() == fresh[-1].tobytes(), 'integral was written without f'
    untouched = all(b.tobytes() == fr.tobytes() for b, fr in zip(back[5:], fresh[5:]))
    res = {name: b[:nr * nx].reshape(nr, nx) for (name, _), b in zip(DENSE, back)}
    res['event_count'] = back[4][:nr].astype(np.int64)
    ne = int(res['event_count'].sum())
    for (name, _, k), b in zip(EVENT, back[5:]):
        res[name] = None if (name == 'integral' and f is None) or rc != 0 else (b[:ne * k].reshape(ne, 2) if k == 2 else b[:ne])
    if first is not None:                                                    # the count-only call wrote the same columns and counts
        for k in range(5):
            assert first[k].tobytes() == back[k].tobytes(), 'count-only and sized call differ in %s' % names[k]
    return rc, res, untouched


def records(ctx, m, periodic, nlev=1):
    q = FR.field(m)
    cnt, ef, et, pts = ctx.contour_segments(q[None], FR.LEVEL, periodic=bool(periodic))
    return cnt.ravel(), ef, et, pts


def scaled(rng, shape, dtype=np.float64, signed=True):
    """values with full mantissas and exponents in [-20, 20]: every term lies wholly inside its window"""
    v = np.ldexp(rng.uniform(1.0, 2.0, shape), rng.integers(-20, 20, shape))
    return (v * rng.choice([-1.0, 1.0], shape) if signed else v).astype(dtype)


def check(ctx, rec, ny, nx, periodic, select, ncont, gap, what='', cap=None, **kw):
    try:
        if cap is not None:
            ctx.set_cpiece_workspace(cap)
        rc, got, _ = call(ctx, *rec, ny, nx, periodic, select, ncont, gap, **kw)
    finally:
        if cap is not None:
            ctx.set_cpiece_workspace(DEFAULT_CAP)
    assert rc == 0, '%s: xc_contour_folds_dev returned %d' % (what, rc)
    ref = FR.folds(*rec, ny, nx, periodic, select, gap=gap, ncont=ncont, **kw)
    bad = FR.differences(got, ref)
    assert bad == [], '%s (periodic %d, select %d, gap %d): %r differ' % (what, periodic, select, gap, bad)
    return got, ref


@pytest.mark.parametrize('name', sorted(CASES))
def test_every_hand_built_plane_with_weights_and_an_integrand(ctx, name):
    """signed float64 weights shared by the slabs and a float64 integrand; then weight 1 without an integrand"""
    m, periodic, select, gap = CASES[name]
    ny, nx = m.shape
    rec = records(ctx, m, periodic)
    rng = np.random.default_rng(len(name) + nx)
    got, ref = check(ctx, rec, ny, nx, periodic, select, 1, gap, name, w=scaled(rng, (ny, nx)), f=scaled(rng, (1, ny, nx)))
    bare, _ = check(ctx, rec, ny, nx, periodic, select, 1, gap, name + ', bare')
    assert bare['integral'] is None and np.array_equal(bare['area'], bare['nodes'].astype(np.float64))
    for k in ('ncross', 'col_event', 'event_count', 'c_west', 'c_east', 'nodes'):
        assert np.array_equal(bare[k], got[k])
    if name == 'seam hook, ring':
        assert got['c_west'].tolist() == [7] and got['c_east'].tolist() == [0]
    if name == 'seam hook, plain':
        assert got['c_west'].tolist() == [0, 7]
    if name.startswith('every column folded'):
        assert got['c_west'].tolist() == [0] and got['ncol'].tolist() == [nx] and (got['col_event'] == 0).all()
    if name == 'blob, main':
        assert got['event_count'].tolist() == [0] and (got['ncross'] == 1).all()
    if name == 'nx 257':
        assert got['c_west'].tolist() == [60, 254] and got['c_east'].tolist() == [69, 1]
    if name == 'ny 300':
        g = IR.scan_geometry(ny, nx, 1)
        assert g['nchunk'] >= 2 and 50 // g['rc'] < 199 // g['rc']          # the fold is cut by the chunks
    if name == 'hook of 3':
        g = IR.scan_geometry(ny, nx, 1)
        assert g['nchunk'] == 2 and g['rc'] == 5                             # the smallest plane already has a cut inside its fold


def stack(ctx, names, periodic, empty=()):
    """the records of several planes of one shape as the ranges of one call, ranges without segments at the positions `empty`"""
    recs, k = [], 0
    n = len(names) + len(empty)
    for i in range(n):
        if i in empty:
            recs.append((np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros((0, 4))))
        else:
            recs.append(records(ctx, CASES[names[k]][0], periodic))
            k += 1
    return tuple(np.concatenate([r[j] for r in recs]) for j in range(4))


def test_six_ranges_in_three_groups_with_empty_ranges_around_and_two_caps(ctx):
    """9 x 8 planes: six ranges with segments, empty ones in front, between and behind; a cap of two table rows gives three groups,
    a cap of one row six, the default one; a per-slab float64 w (two slabs of five ranges) and a float32 integrand"""
    names = ['hook of 3', 'blob, all', 'no fold', 'seam hook, ring', 'every column folded', 'hook of 3']
    ny, nx = 9, 8
    rec = stack(ctx, names, 1, empty=(0, 3, 6, 9))
    assert rec[0].size == 10 and (rec[0] > 0).sum() == 6
    rng = np.random.default_rng(24)
    w, f = scaled(rng, (2, ny, nx)), scaled(rng, (2, ny, nx), np.float32)
    row = 2 * ny * nx * 4
    got, ref = check(ctx, rec, ny, nx, 1, 0, 5, 0, 'default cap', w=w, f=f)
    assert got['event_count'].tolist() == [0, 1, 1, 0, 0, 1, 0, 1, 1, 0]
    for cap, groups in ((2 * row, 3), (row, 6)):
        other, _ = check(ctx, rec, ny, nx, 1, 0, 5, 0, 'cap %d' % cap, cap=cap, w=w, f=f)
        assert FR.differences(other, got) == []
        prof = ctx.last_cfold_profile()
        assert prof['groups'] == groups
    # 'main' on the same ranges: the blob and the band are no part of the main ring
    main, _ = check(ctx, rec, ny, nx, 1, 2, 5, 0, 'main', cap=2 * row, w=w, f=f)
    assert main['event_count'].tolist() == [0, 1, 0, 0, 0, 1, 0, 0, 1, 0]


def test_a_nan_weight_is_skipped_and_an_infinite_one_poisons_its_tongue_alone(ctx):
    m, periodic, select, gap = CASES['two hooks, gap 0']
    ny, nx = m.shape
    rec = records(ctx, m, periodic)
    rng = np.random.default_rng(25)
    w, f = scaled(rng, (ny, nx)), scaled(rng, (1, ny, nx))
    w[2, 2] = np.nan                                                         # under, event 0
    w[5, 3] = np.inf                                                         # over, event 0
    f[0, 1, 5] = -np.inf                                                     # under, event 1: the integral alone
    w[0, 0] = np.inf                                                         # no fold node
    got, ref = check(ctx, rec, ny, nx, periodic, select, 1, gap, 'non-finite', w=w, f=f)
    assert got['nodes'].tolist() == [[4, 4], [4, 6]]
    for k in ('area', 'mx', 'my', 'integral'):
        assert np.isfinite(got[k][0, 0]) and np.isnan(got[k][0, 1]) and np.isfinite(got[k][1, 1])
    assert np.isnan(got['integral'][1, 0]) and np.isfinite(got['area'][1]).all() and np.isfinite(got['my'][1]).all()
    assert FR.same_bits(got['area'][0, 0], math.fsum([w[3, 2], w[2, 3], w[3, 3]]))


def test_capacity_one_short_returns_1_and_leaves_the_event_arrays_alone(ctx):
    m, periodic, select, gap = CASES['two hooks, gap 0']
    ny, nx = m.shape
    rec = records(ctx, m, periodic)
    w = scaled(np.random.default_rng(26), (ny, nx))
    rc, got, untouched = call(ctx, *rec, ny, nx, periodic, select, 1, gap, w=w, capacity=1)
    assert rc == 1 and untouched
    ref = FR.folds(*rec, ny, nx, periodic, select, gap=gap, w=w)
    assert got['event_count'].tolist() == [2] and FR.differences(got, ref, events=False) == []
    rc, got, _ = call(ctx, *rec, ny, nx, periodic, select, 1, gap, w=w, capacity=5)          # room to spare: only two rows are written
    assert rc == 0 and FR.differences(got, ref) == []


def exact_sum_weights(ny, nx, seed):
    """about half the nodes +-2^40, the others full mantissas in [1, 2): adding a small term to a running sum near 2^40 drops 40 of its
    bits, so a plain float64 sum, in whichever order, is not the exact sum rounded once"""
    rng = np.random.default_rng(seed)
    small = rng.uniform(1.0, 2.0, (ny, nx))
    big = rng.choice([2.0 ** 40, -2.0 ** 40], (ny, nx))
    return np.where(rng.random((ny, nx)) < 0.5, big, small)


@pytest.mark.parametrize('name', ['hook of 5', 'every column folded', 'nx 257'])
def test_sums_whose_exact_value_no_summation_order_gives_are_fsum(ctx, name):
    m, periodic, select, gap = CASES[name]
    ny, nx = m.shape
    rec = records(ctx, m, periodic)
    w = exact_sum_weights(ny, nx, 27)
    got, ref = check(ctx, rec, ny, nx, periodic, select, 1, gap, name, w=w)
    # the terms lie inside the window (2^-52 .. 2^41 against a bottom of 2^(53 - 160)), so the reference IS math.fsum; and a plain
    # sum (numpy's pairwise one, Python's sequential one) differs for at least one of the sums of the case
    X = IR.crossing_flags(*rec, ny, nx, periodic, select)[0]
    naive_differs = False
    for e, (cw, ncol) in enumerate(zip(got['c_west'], got['ncol'])):
        cols = [c for c in [(cw + d) % nx for d in range(nx)] if got['col_event'][0, c] == e]
        assert len(cols) == ncol
        terms = [[], []]
        for c in cols:
            rows = np.flatnonzero(X[:, c])
            t = 0
            for r in range(rows[0] + 1, rows[-1] + 1):
                terms[t].append(w[r, c])
                t ^= int(X[r, c])
        for t in (0, 1):
            assert FR.same_bits(got['area'][e, t], math.fsum(terms[t]))
            naive_differs |= float(np.sum(np.array(terms[t]))) != got['area'][e, t] or sum(terms[t]) != got['area'][e, t]
    assert naive_differs


def test_bad_arguments_are_refused(ctx):
    m, periodic, select, gap = CASES['hook of 3']
    ny, nx = m.shape
    rec = records(ctx, m, 1)
    for per, sel, ncont, g in ((0, 1, 1, 0), (0, 2, 1, 0), (1, 3, 1, 0), (1, 0, 0, 0), (1, 0, 2, 0), (1, 2, -1, 0), (1, 2, 1, nx), (1, 2, 1, -1)):
        rc, _, untouched = call(ctx, *rec, ny, nx, per, sel, ncont, g, capacity=4)
        assert rc == nat.XC_EBADARG and untouched, (per, sel, ncont, g)
    bad = rec[1].copy()
    bad[3] = 2 * ny * nx
    rc, _, _ = call(ctx, rec[0], bad, rec[2], rec[3], ny, nx, 1, 2, 1, 0, capacity=4)
    assert rc == nat.XC_EBADARG
    check(ctx, rec, ny, nx, 1, 2, 1, 0, 'the call after the refused one')
