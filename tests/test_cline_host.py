"""The numpy restatement of K15's line-integral rule (cline_ref) pinned on closed forms and on a plane small enough to count by
hand; every case is also shown to fail for a deliberately wrong variant of the rule.  Then the fixed-point model of K15's two sums
(cline_ref.det_integrals) against exact rational sums and its own wrong variants, and the launch model.  No GPU."""
import numpy as np
import pytest

import cline_ref as LR


def row_plane(ny, nx):
    return np.repeat(np.arange(ny, dtype=np.float64)[:, None], nx, axis=1)


def check_row_constant(weight=0.5):
    """q = row index, F = a + b column on a uniform Cartesian grid: a level between two rows is one straight line across the plane,
    the trapezoid rule is exact for a linear integrand: integral = (a + b (nx - 1) / 2) (x[-1] - x[0])"""
    ny, nx, a, b = 6, 9, 3.0, 0.25
    y, x = np.arange(ny) * 2.0, np.arange(nx) * 4.0
    F = a + b * row_plane(nx, ny).T
    lv = np.array([0.5, 2.25, 4.75])
    integ, length, nseg, scale = LR.line_integrals(row_plane(ny, nx), F, lv, y, x, weight=weight)
    assert np.array_equal(nseg, [nx - 1] * 3)
    assert np.array_equal(length, [x[-1] - x[0]] * 3)
    want = (a + b * (nx - 1) / 2) * (x[-1] - x[0])
    assert np.max(np.abs(integ - want)) <= 1e-13 * want
    assert np.array_equal(scale, integ)                      # every term is positive


def test_row_constant_tracer_closed_form():
    check_row_constant()
    with pytest.raises(AssertionError):
        check_row_constant(weight=1.0)                       # trapezoid weight 1 instead of 0.5


def check_constant_integrand(weight=0.5):
    rng = np.random.default_rng(1)
    ny, nx = 23, 31
    q = rng.standard_normal((ny, nx))
    q[rng.random(q.shape) < 0.03] = np.nan
    y, x = np.linspace(0.0, 50.0, ny), np.linspace(0.0, 90.0, nx)
    lv = np.array([-9.0, -1.0, -0.3, 0.0, 0.4, 1.1, np.nan, 9.0])
    for latlon in (False, True):
        yy, xx = (np.deg2rad(y), np.deg2rad(x)) if latlon else (y, x)
        integ, length, nseg, _ = LR.line_integrals(q, np.ones_like(q), lv, yy, xx, latlon, weight=weight)
        rt, rn = LR.CR.contour_lengths_fast(q, lv, yy, xx, latlon)
        assert np.array_equal(nseg, rn) and np.array_equal(length, rt, equal_nan=True)      # K10's own
        assert np.array_equal(np.isnan(length), [True, False, False, False, False, False, True, True])
        assert np.array_equal(integ, length, equal_nan=True)     # (0.5 * 2) * len == len exactly, summed in the same order


def test_constant_integrand_gives_the_length():
    check_constant_integrand()
    with pytest.raises(AssertionError):
        check_constant_integrand(weight=1.0)


def check_nan_skip(nan_as=None):
    """3 x 4 nodes, q = row index.  Level 0.5 runs along row 0.5 through three cells; its four end points lie on the columns'
    vertical edges between rows 0 and 1.  A NaN on node (0, 1) is read by the point on column 1, which the segments of cells 0 and
    1 share: 3 segments -> 1.  Level 1.5 (rows 1 and 2) does not read it.  Level 1.0 lies ON row 1's nodes (case 12, frac 0): its
    points take node (1, c) alone, so a NaN on node (2, 2) -- the other node of their edges -- changes nothing there, and
    takes two of level 1.5's three segments."""
    q = row_plane(3, 4)
    y, x = np.arange(3.0), np.arange(4.0) * 2.0
    F = np.arange(12.0).reshape(3, 4)
    lv = np.array([0.5, 1.0, 1.5])
    clean = LR.line_integrals(q, F, lv, y, x)
    assert np.array_equal(clean[2], [3, 3, 3]) and np.array_equal(clean[1], [6.0, 6.0, 6.0])
    # F on row 0.5: 2 + c; on row 1: 4 + c; on row 1.5: 6 + c; trapezoid over columns 0..3 spaced 2: 2 * sum of the mid values
    assert np.array_equal(clean[0], [2 * (2.5 + 3.5 + 4.5), 2 * (4.5 + 5.5 + 6.5), 2 * (6.5 + 7.5 + 8.5)])
    Fa = F.copy(); Fa[0, 1] = np.nan
    integ, length, nseg, _ = LR.line_integrals(q, Fa, lv, y, x, nan_as=nan_as)
    assert np.array_equal(nseg, [1, 3, 3])
    assert np.array_equal(length, [2.0, 6.0, 6.0])
    assert np.array_equal(integ, [2 * 4.5, clean[0][1], clean[0][2]])
    Fb = F.copy(); Fb[2, 2] = np.nan
    integ, length, nseg, _ = LR.line_integrals(q, Fb, lv, y, x, nan_as=nan_as)
    assert np.array_equal(nseg, [3, 3, 1])
    assert np.array_equal(length, [6.0, 6.0, 2.0])
    assert np.array_equal(integ, [clean[0][0], clean[0][1], 2 * 6.5])


def test_nan_end_point_removes_exactly_its_segments():
    check_nan_skip()
    with pytest.raises(AssertionError):
        check_nan_skip(nan_as=0.0)                           # NaN treated as 0: nothing is skipped


def test_infinite_term_spoils_the_integral_alone():
    q = row_plane(3, 4)
    y, x = np.arange(3.0), np.arange(4.0)
    F = np.ones((3, 4)); F[1, 2] = np.inf
    # level 0.5: node (1, 2) is the SECOND node of its edge: (inf - 1) * 0.5 + 1 = inf: an infinite term.  Level 1.5: it is the
    # first node: (1 - inf) * 0.5 + inf = NaN: the two segments are skipped
    integ, length, nseg, _ = LR.line_integrals(q, F, [0.5, 1.5], y, x)
    assert np.isnan(integ[0]) and length[0] == 3.0 and nseg[0] == 3
    assert integ[1] == 1.0 and length[1] == 1.0 and nseg[1] == 1


def test_periodic_form_is_the_extended_plane():
    rng = np.random.default_rng(2)
    q, F = rng.standard_normal((7, 5)), rng.standard_normal((7, 5))
    y, x = np.arange(7.0), np.arange(5.0) * 3.0
    lv = np.array([-0.5, 0.0, 0.7])
    a = LR.line_integrals_periodic(q, F, lv, y, x, 15.0)
    b = LR.line_integrals(np.hstack([q, q[:, :1]]), np.hstack([F, F[:, :1]]), lv, y, np.append(x, 15.0))
    for u, v in zip(a, b):
        assert np.array_equal(u, v, equal_nan=True)
    assert (a[2] > LR.line_integrals(q, F, lv, y, x)[2]).all()   # the seam cell adds segments


# ---------------------------------------------------------------------------------------------------- the fixed-point model det_integrals
def cut49(v):
    """a float64 cut toward zero to its leading 49 significant bits, as an exact Fraction"""
    import math
    from fractions import Fraction
    m, e = math.frexp(float(v))
    return Fraction(int(abs(m) * 2 ** 53) >> 4, 2 ** 49) * Fraction(2) ** e * (-1 if v < 0 else 1)


@pytest.mark.parametrize('profile', ['mixed', 'cancel'])
def test_model_is_the_exactly_rounded_sum_of_the_cut_terms(profile):
    """where no term reaches the window's last bit the model is: every term cut to 49 bits, the cut terms summed exactly (Fractions),
    the sum rounded once -- and that is not np.sum of the terms"""
    from fractions import Fraction
    q, F, lv, y, x = LR.fixed_point_case(profile, True)
    for s in range(2):
        LR.check_fixed_point_premise(q[s], F[s], lv, y, x)
        k, ln, term = LR.terms(q[s], F[s], lv, y, x)
        integ, length = LR.det_integrals(q[s], F[s], lv, y, x)
        ref = LR.line_integrals(q[s], F[s], lv, y, x)
        assert np.array_equal(np.isnan(integ), np.isnan(ref[0])) and np.array_equal(np.isnan(length), np.isnan(ref[1]))
        for i in np.flatnonzero(~np.isnan(integ)):
            assert integ[i] == float(sum((cut49(t) for t in term[k == i]), Fraction(0)))
            assert length[i] == float(sum((cut49(t) for t in ln[k == i]), Fraction(0)))
        ok = ~np.isnan(integ)
        assert np.all(np.abs(integ[ok] - ref[0][ok]) <= 1e-12 * ref[3][ok])
        if profile == 'cancel':                                  # the residue is out of the 1e-12 bar's sight
            assert np.all(np.abs(ref[0][ok]) < 2.0 ** -40 * ref[3][ok]) and (integ[ok] != 0).all()


@pytest.mark.parametrize('along_x', [True, False])
def test_model_differs_from_np_sum_where_the_window_cuts(along_x):
    """'wide': the lone node of -2^120 sets a window whose last bit (~2^-59) lies inside every term (~2^-30, 49 bits): each drops its
    low chunk, toward zero for both signs.  'under': every term lies under the window, the integral is +0.0 and the length is not NaN"""
    q, F, lv, y, x = LR.fixed_point_case('wide', along_x)
    for s in range(2):
        assert LR.check_fixed_point_premise(q[s], F[s], lv, y, x) > 1000
        k, ln, term = LR.terms(q[s], F[s], lv, y, x)
        assert (term < 0).any() and (term > 0).any()
        integ, length = LR.det_integrals(q[s], F[s], lv, y, x)
        ref = LR.line_integrals(q[s], F[s], lv, y, x)
        ok = ~np.isnan(integ)
        assert ok.sum() > 20 and (integ[ok] != ref[0][ok]).all()
        assert np.array_equal(length, LR.CR.det_totals(q[s], lv, y, x), equal_nan=True)
    q, F, lv, y, x = LR.fixed_point_case('under', along_x)
    for s in range(2):
        integ, length = LR.det_integrals(q[s], F[s], lv, y, x)
        ok = ~np.isnan(length)
        assert ok.sum() > 20 and np.array_equal(np.isnan(integ), ~ok)
        assert (integ[ok] == 0).all() and not np.signbit(integ[ok]).any()


@pytest.mark.parametrize('profile,f_dtype', [(p, np.float64) for p in LR.FP_PROFILES] + [('mixed', np.float32), ('wide', np.float32)])
def test_model_sign_symmetry(profile, f_dtype):
    q, F, lv, y, x = LR.fixed_point_case(profile, profile != 'cancel', f_dtype)
    for s in range(2):
        a = LR.det_integrals(q[s], F[s], lv, y, x, f_dtype=f_dtype)
        b = LR.det_integrals(q[s], -F[s], lv, y, x, f_dtype=f_dtype)
        assert np.array_equal(b[0], -a[0], equal_nan=True)       # (equal nonzero values are equal bits; an empty sum is +0.0 either way)
        assert not np.signbit(a[0][a[0] == 0]).any() and not np.signbit(b[0][b[0] == 0]).any()
        assert np.array_equal(a[1], b[1], equal_nan=True)


# wrong variant -> the profile of fixed_point_case on which it must change bits, and why
WRONG = {'floor': ('wide', 'negative terms drop their low chunk: cut toward minus infinity, each comes out one last bit lower'),
         'max_f': ('wide', 'the largest |F| is the lone NEGATIVE node: max F alone puts the window 150 bits lower, nothing is cut'),
         'nonfinite': ('mixed', 'the lone -inf / NaN node would lift the window above every term: all zero'),
         'len_window': ('wide', 'the length window (top 2^13) keeps every bit of terms of ~2^-30')}


@pytest.mark.parametrize('along_x', [True, False])
@pytest.mark.parametrize('wrong', sorted(WRONG))
def test_wrong_variants_of_the_model_change_bits(wrong, along_x):
    q, F, lv, y, x = LR.fixed_point_case(WRONG[wrong][0], along_x)
    for s in range(2):
        good = LR.det_integrals(q[s], F[s], lv, y, x)
        bad = LR.det_integrals(q[s], F[s], lv, y, x, wrong=wrong)
        ok = ~np.isnan(good[0])
        assert np.array_equal(good[1], bad[1], equal_nan=True) and np.array_equal(np.isnan(bad[0]), ~ok)
        assert (good[0][ok] != bad[0][ok]).mean() > 0.9, WRONG[wrong][1]


def test_model_skips_and_spoils_like_the_restatement():
    """NaN end-point values: skipped in both channels; an infinite term: that level's integral alone is NaN; a slab without a finite
    value has the floor window (bound 0) and no segment; the periodic form is the model on the extended plane"""
    rng = np.random.default_rng(5)
    q, F = rng.standard_normal((9, 12)), rng.standard_normal((9, 12))
    F[rng.random(F.shape) < 0.1] = np.nan
    F[4, 6] = np.inf
    y, x = np.arange(9.0) * 1.5, np.arange(12.0) * 0.75
    lv = np.linspace(-1.0, 1.0, 7)
    integ, length = LR.det_integrals(q, F, lv, y, x)
    ref = LR.line_integrals(q, F, lv, y, x)
    assert np.array_equal(np.isnan(integ), np.isnan(ref[0])) and np.array_equal(np.isnan(length), np.isnan(ref[1]))
    assert (np.isnan(integ) & ~np.isnan(length)).any()
    ok = ~np.isnan(integ)
    assert np.all(np.abs(integ[ok] - ref[0][ok]) <= 1e-12 * ref[3][ok]) and np.allclose(length, ref[1], rtol=1e-12, atol=0, equal_nan=True)
    a, b = LR.det_integrals(q, np.full_like(F, np.nan), lv, y, x)
    assert np.isnan(a).all() and np.isnan(b).all()
    import xcontour_oracle as O
    assert LR.term_window_top(np.full((3, 3), np.nan), 2.0) == O.DET_TOP_FLOOR == LR.term_window_top(np.zeros((3, 3)), 2.0)
    assert LR.term_window_top(np.array([[-3.0, 1.0, np.inf]]), 2.0) == 3 + O.DET_TOP_SLACK                      # 6.0000006 < 2^3
    assert LR.term_window_top(np.array([[1e-40]]), 1.0, np.float32) == O.det_window_top(float(np.float32(1e-40)) * 1.0000001)
    F[np.isnan(F)] = 0.25
    p = LR.det_integrals(q, F, lv, y, x, period=9.0)
    e = LR.det_integrals(np.hstack([q, q[:, :1]]), np.hstack([F, F[:, :1]]), lv, y, np.append(x, 9.0))
    assert np.array_equal(p[0], e[0], equal_nan=True) and np.array_equal(p[1], e[1], equal_nan=True)


# ---------------------------------------------------------------------------------------------------- the launch model
def test_launch_model_thresholds():
    """K15 (10 words, 16383 cells per LDS copy): 8 copies up to N = 72, 4 up to 142, 2 up to 279, 1 past that, level groups of 533;
    a block may walk 15 / 7 / 3 / 1 tiles.  K10 (5 words, 32767 cells): 136 / 266 / 511, groups of 944, 31 / 15 / 7 / 3 tiles"""
    geo = lambda N, **kw: LR.CR.launch_geometry(N, 33, 64, 1, **kw)
    k15 = dict(words=10, copy_cells=16383)
    for N, ncopy, G, ngroup in [(1, 8, 1, 1), (72, 8, 72, 1), (73, 4, 73, 1), (142, 4, 142, 1), (143, 2, 143, 1), (279, 2, 279, 1),
                                (280, 1, 280, 1), (533, 1, 533, 1), (534, 1, 533, 2), (1066, 1, 533, 2), (1067, 1, 533, 3)]:
        g = geo(N, **k15)
        assert (g['ncopy'], g['G'], g['ngroup']) == (ncopy, G, ngroup), N
    for N, ncopy, ngroup in [(136, 8, 1), (137, 4, 1), (266, 4, 1), (267, 2, 1), (511, 2, 1), (512, 1, 1), (944, 1, 1), (945, 1, 2)]:
        g = geo(N)
        assert (g['ncopy'], g['ngroup'], g['G']) == (ncopy, ngroup, min(N, 944)), N
    # tiles per block from the capacity rule: 256 slabs (share 8), 40 tile rows: bps = ceil(40 / max_tiles)
    for N, kw, max_tiles in [(72, k15, 15), (142, k15, 7), (279, k15, 3), (280, k15, 1), (136, {}, 31), (266, {}, 15), (511, {}, 7), (512, {}, 3)]:
        g = LR.CR.launch_geometry(N, 40 * 32 + 1, 2, 256, **kw)
        assert g['ntile'] == 40 and g['bps'] == max(8, -(-40 // max_tiles)), (N, g)
        assert g['bps_rule'] == ('capacity' if -(-40 // max_tiles) > 8 else 'share')
    # the four rules, a ring's extra cell column, planes without cells
    assert LR.CR.launch_geometry(40, 258, 40, 256, **k15)['bps_rule'] == 'share'
    assert LR.CR.launch_geometry(40, 258, 40, 300, **k15)['bps_rule'] == 'floor'
    assert LR.CR.launch_geometry(300, 961, 2, 256, **k15) == dict(N=300, ncopy=1, G=300, ngroup=1, ntile=30, bps=30, bps_rule='capacity', nslab=256)
    assert LR.CR.launch_geometry(150, 961, 2, 256, **k15)['bps'] == 10
    assert LR.CR.launch_geometry(40, 33, 64, 1, **k15)['bps_rule'] == 'ntile'
    assert LR.CR.launch_geometry(9, 33, 252, 1, wrap=True, **k15)['ntile'] == 1 and LR.CR.launch_geometry(9, 33, 253, 1, wrap=True, **k15)['ntile'] == 2
    assert LR.CR.launch_geometry(9, 33, 253, 1, **k15)['ntile'] == 1
    for ny, nx in [(1, 40), (30, 1), (1, 1)]:
        g = LR.CR.launch_geometry(3, ny, nx, 3, **k15)
        assert (g['ntile'], g['bps'], g['bps_rule']) == (0, 0, None)
