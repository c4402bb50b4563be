"""The numpy restatement of K15's line-integral rule (cline_ref) pinned on closed forms and on a plane small enough to count by
hand; every case is also shown to fail for a deliberately wrong variant of the rule.  No GPU."""
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
