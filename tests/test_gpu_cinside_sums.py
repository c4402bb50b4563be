"""The sums of K17 (xc_contour_interior_dev) and K18 (xc_contour_piece_interiors_dev) at the edges of their windows, BIT FOR BIT against
cinside_ref.interior and cpinside_ref.piece_interiors, which state the header's rule (include/xcontour_hip.h, K17 section): a window of
160 bits under 2^top, top = 12 + the frexp exponent of the largest finite |w| (|w f|) of the slab's plane, never below -800; the bits of
a term under 2^(top - 160) cut off toward zero; a NaN term skipped, an infinite one making that sum NaN.  The records suites
(test_gpu_cinside_records.py, test_gpu_cpinside_records.py) keep every term in the middle of its window; here the terms are chosen:
ties, sticky bits, borrows, every shift against the limb grid, the window's bottom, a bound far from the terms, non-finite values that
must not lift the window, the floor of the window, a bound near 2^1000, windows that differ per slab, a float32 integrand, and hundreds
of equal terms.  Both kernels keep the limbs in registers (cp_add_private), K17 with a 64-lane butterfly behind it, and both derive the
windows on the device (k_ci_bound, ci_top): none of that is reached by K13's suite.

cinside_sums_cases.py holds the planes, the term lists and the placements; test_cinside_host.py and test_cpinside_host.py show on the
CPU that the reference is the limb model on these very lists, and which broken accumulator or bound rule each list catches.  Every
call goes through call / check of the two records suites: guards behind every output, n_in and K17's mask equal, the sums equal bit for
bit; no tolerance anywhere.  Every K17 call is repeated with one range per group (cap = 1), every K18 call with its records shuffled.
Not pinned here: a sum that overflows float64 -- the header does not define it; the high-bound cases keep |sum| < 2^1020."""
import math

import numpy as np
import pytest

import cinside_ref as IR
import cinside_sums_cases as SC
import test_gpu_cinside_records as T17
import test_gpu_cpinside_records as T18

pytestmark = pytest.mark.gpu


def run_both(ctx, pl, nslab, what, w=None, f=None):
    """one call on pl's records, once per slab, checked against the reference in full -> (sum_w, sum_wf, n_in per range, tops per slab)"""
    rec = SC.records(pl, nslab)
    ny, nx, periodic, flip, nlev = pl['ny'], pl['nx'], pl['periodic'], pl['flip'], pl['nlev']
    tops = IR.window_tops(w, f, nslab, ny, nx)
    if pl['kind'] == 'k17 rows':
        got, ref = T17.check(ctx, rec, ny, nx, periodic, pl['select'], flip, nlev, what, w=w, f=f)
        one = T17.run(ctx, rec, ny, nx, periodic, pl['select'], flip, nlev, cap=1, w=w, f=f)
        assert T17.differences(one, got) == [], what + ': one range per group against one group'
        assert ref['tops'] == tops and np.array_equal(got['mask'], np.tile(pl['masks'], (nslab, 1, 1)))
        return got['sum_w'], got['sum_wf'], got['n_in'], tops
    got = T18.check(ctx, rec, ny, nx, periodic, flip, nlev, what, w=w, f=f)
    assert all(t.size == 1 and t['closed'][0] for t in got), what
    assert T18.same(T18.tables(ctx, T18.shuffled(rec, 7), ny, nx, periodic, flip, nlev, cap=1, w=w, f=f), got), what + ': shuffled, one range per group'
    assert T18.same(T18.tables(ctx, T18.shuffled(rec, 8), ny, nx, periodic, flip, nlev, w=w, f=f), got), what + ': shuffled'
    return (np.array([t['sum_w'][0] for t in got]), None if f is None else np.array([t['sum_wf'][0] for t in got]),
            np.array([t['n_in'][0] for t in got]), tops)


def count_inside(pl, nslab):
    return np.tile(pl['masks'].reshape(pl['nlev'], -1).sum(axis=1), nslab).tolist()


@pytest.mark.parametrize('batch', sorted(SC.batches()))
@pytest.mark.parametrize('kind', SC.KINDS)
def test_term_lists_in_w_in_a_float64_f_and_in_a_float32_f(ctx, kind, batch):
    """every list of the batch, one per slab, in every placement on 12 x 70 and 70 x 12 (a taller or 70 x 70 plane where a list does not
    fit); the windows are the ones the case names, the written-out sums are returned, and a case about the cut differs from plain fsum"""
    ran = 0
    for what, pl, W, cases in SC.runs(kind, batch):
        for vname, w, f, which in SC.variants(W, cases):
            sw, swf, n_in, tops = run_both(ctx, pl, len(which), '%s, %s' % (what, vname), w=w, f=f)
            assert n_in.tolist() == count_inside(pl, len(which))
            got = sw if vname == 'w' else swf
            for j, k in enumerate(which):
                cs, where = cases[k], (what, vname, cases[k]['name'])
                assert tops[j][0 if vname == 'w' else 1] == cs['top'] and tops[j][0] == (cs['top'] if vname == 'w' else SC.TOP), where
                terms = [t for t in SC.inside_terms(pl, W, k) if not math.isnan(t)]
                if any(math.isinf(t) for t in terms):
                    assert math.isnan(got[j]), where
                    continue
                if cs['want'] is not None:
                    assert SC.same(got[j], cs['want']), where
                assert (not SC.same(got[j], math.fsum(terms))) == cs['cut'], where
                if vname != 'w':
                    assert sw[j] == n_in[j], where                           # weight 1
            ran += 1
    assert ran >= 2


@pytest.mark.parametrize('shape', SC.SHAPES, ids=['%dx%d' % s for s in SC.SHAPES])
@pytest.mark.parametrize('kind', SC.KINDS)
def test_the_floor_of_the_window(ctx, kind, shape):
    """zero, denormal and NaN weights give +0.0 and leave n_in alone; under a largest weight of 2^-900 the window stands at its floor
    (top -800, bottom -960): terms at 2^-900 survive, a term at 2^-1000 and a denormal product are dropped"""
    pl = SC.plane(kind, *shape)
    for name, w, f, want in SC.floor_case(pl):
        sw, swf, n_in, tops = run_both(ctx, pl, 1, 'floor: ' + name, w=w, f=f)
        assert tops == [(-800, -800)] and n_in.tolist() == count_inside(pl, 1), name
        assert SC.same(sw[0], want['sum_w']) and SC.same(swf[0], want['sum_wf']), name
        sw, _, _, _ = run_both(ctx, pl, 1, 'floor, no f: ' + name, w=w)
        assert SC.same(sw[0], want['sum_w']), name


@pytest.mark.parametrize('shape', SC.SHAPES, ids=['%dx%d' % s for s in SC.SHAPES])
@pytest.mark.parametrize('kind', SC.KINDS)
def test_every_slab_has_its_own_windows_and_both_ranges_of_a_slab_use_them(ctx, kind, shape):
    """two slabs 2^120 apart, the sticky tie inside each, two ranges per slab (ncont 2): a window taken from the other slab, or the
    window of w f taken from w, loses the sticky bit or overflows"""
    pl = SC.plane(kind, *shape, nlev=2)
    for what in ('f', 'w'):
        w, f, want_tops, want = SC.per_slab_case(pl, what)
        sw, swf, n_in, tops = run_both(ctx, pl, 2, 'per-slab windows in ' + what, w=w, f=f)
        assert tops == want_tops and n_in.tolist() == count_inside(pl, 2)
        got = swf if what == 'f' else sw
        assert SC.same(got, [want[0], want[0], want[1], want[1]])


@pytest.mark.parametrize('shape', SC.SHAPES, ids=['%dx%d' % s for s in SC.SHAPES])
@pytest.mark.parametrize('kind', SC.KINDS)
def test_a_float32_integrand_is_cast_before_the_product_and_an_overflowing_product_lifts_no_window(ctx, kind, shape):
    pl = SC.plane(kind, *shape)
    m = pl['masks'][0]
    w, f = SC.float32_integrand_case(pl)
    _, swf, _, _ = run_both(ctx, pl, 1, 'float32 integrand', w=w, f=f)
    cast_after = (w * f[0].astype(np.float64)).astype(np.float32).astype(np.float64)
    in_float32 = (w.astype(np.float32) * f[0]).astype(np.float64)
    assert f.dtype == np.float32 and SC.same(swf[0], math.fsum((w * f[0].astype(np.float64))[m]))
    assert not SC.same(swf[0], math.fsum(cast_after[m])) and not SC.same(swf[0], math.fsum(in_float32[m]))
    for inside in (False, True):
        w, f = SC.overflow_case(pl, inside)
        sw, swf, _, tops = run_both(ctx, pl, 1, 'w f overflows %s' % ('inside' if inside else 'outside'), w=w, f=f)
        assert tops[0][0] == 1013 and 0 < tops[0][1] <= 53
        assert np.isnan(swf[0]) == inside and SC.same(sw[0], 2.0 ** 1000 if inside else 0.0)
        if not inside:
            with np.errstate(over='ignore'):
                assert SC.same(swf[0], math.fsum((w * f[0])[m]))
