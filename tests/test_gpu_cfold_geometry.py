"""xc_contour_folds_dev (K24) at the boundaries of its launch geometry, against cfold_ref.folds: integers equal, rows and all four sums
BIT FOR BIT, nothing compared with a tolerance.  The planes are cfold_geometry_cases' (test_cfold_geometry_host.py shows on the CPU that
each lies on the boundary its tag names): gaps on a wave and a tile edge of the run pass, tiles without folded column, the seam
renumbering with three and four heads, ranges whose staging slots are all taken, 32 events in every wave of the fold scan, events several
waves and workgroups add up, one to thirteen chunks of rows, and 300 ranges in one call.  The records are K12's own
(Context.contour_segments); the calls go through the guarded-output call / check of test_gpu_cfold_records.py, so every call is a
count-only call and a sized one whose dense outputs agree, with patterns and guards behind every array.

Every case runs twice: with signed float64 weights whose terms lie wholly inside their windows (exponents in [-20, 20], dx < 1000) and
an integrand, and bare.  The calls of several ranges run again under a cap of one table row: one group per range with segments."""
import math

import numpy as np
import pytest

import cfold_geometry_cases as GC
import cfold_ref as FR
import cinside_ref as IR
import test_gpu_cfold_records as T24

pytestmark = pytest.mark.gpu

CASES = GC.cases()


def records(ctx, case):
    return GC.stacked(case, lambda m: T24.records(ctx, m, case.periodic))


def weights(case, name):
    """-> (w, f): w shared by the slabs (per slab on 'many ranges'), f float64 (float32 on 'many ranges')"""
    ny, nx = GC.shape(case)
    nslab = len(case.masks) // case.ncont
    rng = np.random.default_rng(len(name) + nx)
    many = name == 'many ranges'
    return T24.scaled(rng, (nslab, ny, nx) if many else (ny, nx)), T24.scaled(rng, (nslab, ny, nx), np.float32 if many else np.float64)


def events_of(out, r):
    a = int(out['event_count'][:r].sum())
    b = a + int(out['event_count'][r])
    return list(zip(out['c_west'][a:b].tolist(), out['c_east'][a:b].tolist(), out['ncol'][a:b].tolist()))


@pytest.mark.parametrize('name', sorted(CASES))
def test_every_plane_of_the_geometry_with_weights_and_an_integrand_and_bare(ctx, name):
    case = CASES[name]
    ny, nx = GC.shape(case)
    nr = len(case.masks)
    rec = records(ctx, case)
    assert rec[0].size == nr and [int(c) > 0 for c in rec[0]] == [m is not None for m in case.masks]
    geo = IR.scan_geometry(ny, nx, nr)
    assert all(geo[k] == v for k, v in case.pins.items() if k in ('nchunk', 'rc'))
    w, f = weights(case, name)
    args = (ny, nx, case.periodic, case.select, case.ncont, case.gap)
    got, ref = T24.check(ctx, rec, *args, name, w=w, f=f)
    bare, _ = T24.check(ctx, rec, *args, name + ', bare')
    assert bare['integral'] is None and np.array_equal(bare['area'], bare['nodes'].astype(np.float64))
    for k in ('ncross', 'col_event', 'event_count', 'c_west', 'c_east', 'ncol', 'nodes'):
        assert np.array_equal(bare[k], got[k]), k
    for r, drawn in enumerate(case.events):                                  # the events the planes were drawn with
        assert events_of(got, r) == drawn, (name, r)
    if case.pins.get('full'):
        assert got['event_count'][0] == (nx + 1) // 2
    if name.startswith('comb') and case.gap == 0:
        # the reductions of the events of one wave are not mixed: neighbouring events (every other lane) have sums of their own, in
        # both tongues (mx is 0: every event is one column)
        n0 = int(got['event_count'][0])
        assert not got['mx'][:n0].any()
        for k in ('area', 'my', 'integral'):
            v = got[k][:n0]
            assert (v[1:] != v[:-1]).all(), k
        assert (got['nodes'][:n0] == [1, 2]).all()
    if nr == 1:
        return
    # one range per group: a cap of one row of the edge table (2 ny nx ints)
    assert ctx.last_cfold_profile()['groups'] == 1
    row = 2 * ny * nx * 4
    other, _ = T24.check(ctx, rec, *args, name + ', one range per group', cap=row, w=w, f=f)
    assert ctx.last_cfold_profile()['groups'] == int((rec[0] > 0).sum())
    assert FR.differences(other, got) == []
    other, _ = T24.check(ctx, rec, *args, name + ', bare, one range per group', cap=row)
    assert ctx.last_cfold_profile()['groups'] == int((rec[0] > 0).sum())
    assert FR.differences(other, bare) == []


def test_the_wide_hook_adds_its_limbs_from_five_waves_to_the_exact_sum(ctx):
    """one event over the columns 40 .. 300: five waves of two workgroups (times two chunks of rows) add their limbs with atomics.  On
    weights of +-2^40 mixed with [1, 2) the terms lie inside the window (2^-52 .. 2^41 against a bottom of 2^(53 - 160)), so the
    reference IS math.fsum, and no plain float64 sum gives it."""
    case = CASES['wide hook']
    ny, nx = GC.shape(case)
    rec = records(ctx, case)
    w = T24.exact_sum_weights(ny, nx, 28)
    got, ref = T24.check(ctx, rec, ny, nx, case.periodic, case.select, 1, case.gap, 'wide hook, exact sums', w=w)
    assert events_of(got, 0) == [(40, 300, 261)]
    X = IR.crossing_flags(*rec, ny, nx, case.periodic, case.select)[0]
    terms = [[], []]
    for c in range(40, 301):
        rows = np.flatnonzero(X[:, c])
        t = 0
        for r in range(rows[0] + 1, rows[-1] + 1):
            terms[t].append(w[r, c])
            t ^= int(X[r, c])
    assert [len(t) for t in terms] == got['nodes'][0].tolist() == [522, 522]
    naive_differs = False
    for t in (0, 1):
        assert FR.same_bits(got['area'][0, t], math.fsum(terms[t]))
        naive_differs |= float(np.sum(np.array(terms[t]))) != got['area'][0, t] or sum(terms[t]) != got['area'][0, t]
    assert naive_differs
