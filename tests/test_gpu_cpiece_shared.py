"""K13, K14, K16, K17 and K18 (xc_contour_pieces_dev, xc_contour_polylines_dev, xc_contour_overturning_dev, xc_contour_interior_dev,
xc_contour_piece_interiors_dev) on ONE context in every order: the five entries run phase A on the context's one workspace, each with a
layout of its own in front of the common tail, and each keeps a profile record of its own.  Every result of every call of all 120 orders
is BITWISE the result of the same call on a context that has done nothing else, and after each sequence every entry's profile reports its
own call's groups and rounds, whichever entry ran last.  The reference side is the library itself on a fresh context: no tolerance, no
CPU oracle.

The input is test_gpu_cprecords_shared.py's: a stack of four 24 x 65 planes, periodic and plain, at three levels of which the middle one
has no segments: twelve ranges, every third one empty, the records of every range shuffled.  The five entries run under five caps of the
edge tables -- 1, 2, 3, 4 and 6 table rows -- which cut the twelve ranges into 8, 5, 4, 3 and 2 groups (cp_plan_groups: empty ranges in
front of a group and behind it cost no row; under two rows the ranges 0 and 11 stand alone), so that a profile that took another entry's
count shows.  K16 and K17 select every piece on the plain plane and the main ring on the periodic one.  K13's and K18's rows come in the
order their roots were counted, which is the call's own: they are compared sorted by first_edge; the other outputs are dense or in walk
order and compared as they are, guard elements included.

The last case puts a K14 call that is refused for a repeated edge id between two K13 calls, under kernel timing.  A refused K14 call has
run every group before the error word is read, so its profile holds its own groups and rounds (the library has always reported them;
they are compared to the same refused call on a fresh context) -- what must not happen is that it touches K13's record or leaves a
table behind on which the next call goes wrong.

The case behind it runs K24, K22 and K23 (contour_folds, label_overlap, ring_tracks) between K13, K16 and K17 through the package's
methods, on inputs of two sizes: all six lay out the context's two grow-only workspaces, each in its own way, and a layout that is
smaller than the one before it, or larger, must come out the same."""
import itertools

import numpy as np
import pytest

import cptree_cases as CS
import test_gpu_cinside_records as K17
import test_gpu_cjoin_records as K14
import test_gpu_coverturn_records as K16
import test_gpu_cpiece_records as K13
import test_gpu_cpinside_records as K18
from test_gpu_cpinside_records import DEFAULT_CAP, scaled, shuffled, trace
from test_gpu_cprecords_shared import LEVELS, NSLAB, NX, NY, ROW, canonical
from xcontour_amd import _native as nat

pytestmark = pytest.mark.gpu

# entry -> (table rows under its cap, the groups that makes of the twelve ranges)
PLAN = {'pieces': (1, 8), 'polylines': (2, 5), 'overturning': (3, 4), 'interior': (4, 3), 'interiors': (6, 2)}
PROFILE = {'pieces': 'last_cpiece_profile', 'polylines': 'last_cjoin_profile', 'overturning': 'last_coverturn_profile',
           'interior': 'last_cinterior_profile', 'interiors': 'last_cpinside_profile'}
YC, XC = np.arange(NY, dtype=np.float64), np.arange(NX, dtype=np.float64)


def as_bytes(values):
    return [b'' if v is None else np.ascontiguousarray(v).tobytes() for v in values]


def profile(ctx, entry):
    p = getattr(ctx, PROFILE[entry])()
    return p['groups'], p['rounds']


def run(ctx, entry, rec, periodic, w, f, rows=None):
    """one call of `entry` under its cap (or one of `rows` table rows) -> (the bytes of everything it returned, (groups, rounds) of its
    profile)"""
    select = 2 if periodic else 0
    ctx.set_cpiece_workspace((rows or PLAN[entry][0]) * ROW)
    try:
        if entry == 'pieces':
            got = as_bytes(K13.run_records(ctx, *rec[:4], NY, NX, YC, XC, periodic, float(NX) if periodic else 0.0))
        elif entry == 'polylines':
            rc, out = K14.call_dev(ctx, *rec[:4], ny=NY, nx=NX)
            assert rc == 0, 'polylines returned %d' % rc
            got = as_bytes(out[k] for k in sorted(out))
        elif entry == 'overturning':
            rc, out, _ = K16.call_records(ctx, *rec[:4], NY, NX, periodic, select)
            assert rc == 0, 'overturning returned %d' % rc
            got = as_bytes(out.values())
        elif entry == 'interior':
            rc, out, _ = K17.call(ctx, *rec[:4], NY, NX, periodic, select, 1, len(LEVELS), w=w, f=f)
            assert rc == 0, 'interior returned %d' % rc
            got = as_bytes(out[k] for k in sorted(out))
        else:
            rc, pc, cols, _ = K18.call(ctx, *rec[:4], NY, NX, periodic, 0, len(LEVELS), w=w, f=f)
            assert rc == 0, 'interiors returned %d' % rc
            got = canonical(pc, cols)
    finally:
        ctx.set_cpiece_workspace(DEFAULT_CAP)
    return got, profile(ctx, entry)


def alone(entry, rec, periodic, w, f, rows=None):
    """the same call on a context that has done nothing else"""
    fresh = nat.Context(0)
    try:
        fresh.set_kernel_timing(True)
        return run(fresh, entry, rec, periodic, w, f, rows)
    finally:
        fresh.close()


def records(periodic):
    q = np.stack([CS.smooth_noise(NY, NX, 300 + s) for s in range(NSLAB)])
    rec = shuffled(trace(q, periodic, LEVELS), 17)
    assert (rec[0].reshape(NSLAB, 3) > 0).tolist() == [[True, False, True]] * NSLAB
    rng = np.random.default_rng(23)
    return rec, scaled(rng, (NSLAB, NY, NX)), scaled(rng, (NSLAB, NY, NX), np.float32)


@pytest.mark.parametrize('periodic', [0, 1], ids=['plain', 'ring'])
def test_the_five_entries_in_all_120_orders_on_one_context(ctx, periodic):
    rec, w, f = records(periodic)
    ctx.set_kernel_timing(True)
    try:
        want = {entry: alone(entry, rec, periodic, w, f) for entry in PLAN}
        for entry, (_, (groups, rounds)) in want.items():
            assert groups == PLAN[entry][1], (entry, groups)
            assert rounds >= groups, (entry, rounds)
        assert len({p[0] for _, p in want.values()}) == 5                    # five different group counts
        # K14 does the label rounds and as many rank rounds: twice K13's under the same cap
        for rows in (1, 2):
            k13, k14 = alone('pieces', rec, periodic, w, f, rows)[1], alone('polylines', rec, periodic, w, f, rows)[1]
            assert k14 == (k13[0], 2 * k13[1]), (rows, k13, k14)
        for order in itertools.permutations(PLAN):
            for entry in order:
                got, _ = run(ctx, entry, rec, periodic, w, f)
                assert got == want[entry][0], '%s in the order %s is not what it is alone' % (entry, ' '.join(order))
            for entry in PLAN:                                               # after the sequence: every profile still its own call's
                assert profile(ctx, entry) == want[entry][1], (entry, order)
    finally:
        ctx.set_kernel_timing(False)


def test_a_refused_polylines_call_between_two_pieces_calls(ctx):
    rec, w, f = records(1)
    cnt, ef, et, pts = rec[:4]
    bad = ef.copy()
    bad[1] = bad[0]                                                          # a repeated e_from in range 0
    rows = 2

    def refused(c):
        c.set_cpiece_workspace(rows * ROW)
        try:
            rc, out = K14.call_dev(c, cnt, bad, et, pts, ny=NY, nx=NX)
        finally:
            c.set_cpiece_workspace(DEFAULT_CAP)
        assert rc == nat.XC_EBADARG
        assert 'an edge id repeats' in (c.lib.xc_last_error(c.handle) or b'').decode()
        K14.untouched(out, 'poly_count')
        return profile(c, 'polylines')

    ctx.set_kernel_timing(True)
    try:
        want, k13 = alone('pieces', rec, 1, w, f, rows)
        fresh = nat.Context(0)
        try:
            fresh.set_kernel_timing(True)
            its_own = refused(fresh)
        finally:
            fresh.close()
        print('the refused call alone: groups %d rounds %d' % its_own)
        assert its_own == (k13[0], 2 * k13[1])                               # every group ran before the word was read
        got, prof = run(ctx, 'pieces', rec, 1, w, f, rows)
        assert got == want and prof == k13
        assert refused(ctx) == its_own
        assert profile(ctx, 'pieces') == k13, 'the refused call wrote into the profile of K13'
        got, prof = run(ctx, 'pieces', rec, 1, w, f, rows)
        assert got == want, 'the call after the refused one is not what it is alone'
        assert prof == k13
        assert profile(ctx, 'polylines') == its_own
    finally:
        ctx.set_kernel_timing(False)


# ------------------------------------------------------------------ K24, K22 and K23 between K13, K16 and K17: layouts of different sizes
LEV3 = np.array([-0.4, 0.1, 0.5])
SIZES = {'large': (2, 24, 40), 'small': (1, 6, 8)}
ENTRIES = ('folds', 'pieces', 'overlap', 'overturning', 'tracks', 'interior')
ORDERS = {'small then large': [(e, s) for s in ('small', 'large') for e in ENTRIES],
          'large then small': [(e, s) for s in ('large', 'small') for e in ENTRIES],
          'alternating': [(e, ('small', 'large')[(k + j) % 2]) for j in range(2) for k, e in enumerate(ENTRIES)]}


def flat(out):
    """the bytes of whatever a method returned: arrays, None, tuples and dicts of them"""
    if isinstance(out, dict):
        return [(k, flat(out[k])) for k in sorted(out)]
    if isinstance(out, (tuple, list)):
        return [flat(v) for v in out]
    return b'' if out is None else np.ascontiguousarray(out).tobytes()


def ring_graph(nring, nlink, seed):
    """rings in steps of about eight, links between the rings of consecutive steps: ring_step, ring_size, link_a, link_b, link_n"""
    rng = np.random.default_rng(seed)
    step = (np.arange(nring) // 8).astype(np.int32)
    size = rng.integers(1, 50, nring).astype(np.int64)
    a = rng.integers(0, max(1, nring - 8), nlink).astype(np.int64)
    b = np.minimum(a + rng.integers(1, 9, nlink), nring - 1).astype(np.int64)
    return step, size, a, b, rng.integers(0, 40, nlink).astype(np.int64)


def inputs(size, periodic):
    """the fields, weights, label maps (K20's, made on a context of their own) and the ring graph of one size"""
    ns, ny, nx = SIZES[size]
    seed = 500 + ny
    q, q2 = (np.stack([CS.smooth_noise(ny, nx, seed + 10 * k + s) for s in range(ns)]) for k in range(2))
    rng = np.random.default_rng(seed)
    d = {'q': q, 'w': scaled(rng, (ns, ny, nx)), 'f': scaled(rng, (ns, ny, nx), np.float32),
         'yc': np.arange(ny, dtype=np.float64), 'xc': np.arange(nx, dtype=np.float64), 'ny': ny, 'nx': nx,
         'graph': ring_graph(700, 900, seed) if size == 'large' else ring_graph(5, 4, seed)}
    maker = nat.Context(0)
    try:
        d['la'], d['lb'] = (maker.contour_piece_labels(v, LEV3, periodic=bool(periodic))[2] for v in (q, q2))
    finally:
        maker.close()
    return d


def one_call(c, entry, d, periodic, rows):
    """`entry` through the package's method under a cap of `rows` table rows of the call's own plane -> the bytes of all it returned"""
    per, sel = bool(periodic), 'main' if periodic else 'all'
    c.set_cpiece_workspace(rows * 2 * d['ny'] * d['nx'] * 4)
    try:
        if entry == 'folds':
            out = c.contour_folds(d['q'], LEV3, w=d['w'], f=d['f'], periodic=per, select=sel, gap=1)
        elif entry == 'pieces':
            out = c.contour_pieces(d['q'], LEV3, d['yc'], d['xc'], period=float(d['nx']) if per else None)
        elif entry == 'overlap':
            out = c.label_overlap(d['la'], d['lb'], w=d['w'], f=d['f'])
        elif entry == 'overturning':
            out = c.contour_overturning(d['q'], LEV3, periodic=per, select=sel)
        elif entry == 'tracks':
            out = c.ring_tracks(*d['graph'], min_overlap=0.3)
        else:
            out = c.contour_interior(d['q'], LEV3, w=d['w'], f=d['f'], periodic=per, select=sel, return_mask=True)
    finally:
        c.set_cpiece_workspace(DEFAULT_CAP)
    return flat(out)


@pytest.mark.parametrize('periodic', [0, 1], ids=['plain', 'ring'])
def test_folds_overlap_and_tracks_between_the_piece_entries_on_one_context(ctx, periodic):
    """K24, K22 and K23 interleaved with K13, K16 and K17 on one context, on two slabs of 24 x 40 and on one of 6 x 8 at three levels,
    under caps of 1 and 2 table rows: the grow-only workspaces are reused by layouts of different sizes, small after large and large
    after small.  Every result is bitwise that of the same call on a context that has done nothing else."""
    data = {size: inputs(size, periodic) for size in SIZES}
    want = {}
    for rows in (1, 2):
        for size in SIZES:
            for entry in ENTRIES:
                fresh = nat.Context(0)
                try:
                    want[entry, size, rows] = one_call(fresh, entry, data[size], periodic, rows)
                    if entry == 'folds' and size == 'large':                 # several groups, the rows cut into several chunks
                        assert fresh.last_cfold_profile()['groups'] > 1
                finally:
                    fresh.close()
    assert data['large']['ny'] >= 2 * 4                                      # (ci_geometry: chunks of four rows or more)
    for rows in (1, 2):
        for name, order in ORDERS.items():
            for entry, size in order:
                got = one_call(ctx, entry, data[size], periodic, rows)
                assert got == want[entry, size, rows], '%s (%s) in the order "%s" under %d rows is not what it is alone' % (entry, size, name, rows)
