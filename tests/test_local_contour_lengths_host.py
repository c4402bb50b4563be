"""Contour2D.cal_local_contour_lengths without a GPU: the entry points exist, the facade rejects what it cannot take, and the numpy
restatement of the windows (local_clength_ref) meets closed forms."""
import math

import numpy as np
import pytest

import clength_ref as CR
import local_clength_ref as LR
import xcontour_amd as xa
from xcontour_amd import _native as nat


def test_entry_points_exist():
    assert callable(getattr(xa.Contour2D, 'cal_local_contour_lengths', None))
    assert callable(getattr(nat.Context, 'local_contour_lengths', None))
    for name in ('xc_local_contour_lengths', 'xc_local_contour_lengths_dev'):
        assert name in nat.PROTOTYPES


def test_facade_rejects_plane_without_coordinates_and_small_windows():
    q = xa.DataArray(np.zeros((4, 6)), ('lat', 'lon'), {'lat': np.arange(4.)}, 'q')
    cm = xa.Contour2D(q, np.ones(4), {'X': 'lon', 'Y': 'lat'}, {'Y': 'lat'})
    with pytest.raises(Exception, match='coordinate values for the plane dim lon'):
        cm.cal_local_contour_lengths(3)
    q = xa.DataArray(np.zeros((4, 6)), ('lat', 'lon'), {'lat': np.arange(4.), 'lon': np.arange(6.)}, 'q')
    cm = xa.Contour2D(q, np.ones(4), {'X': 'lon', 'Y': 'lat'}, {'Y': 'lat'})
    for bad in (1, {'lat': 3, 'lon': 1}):
        with pytest.raises(Exception, match='window should be at least 2'):
            cm.cal_local_contour_lengths(bad)
    with pytest.raises(Exception, match='stride should be at least 1'):
        cm.cal_local_contour_lengths(3, stride=0)
    with pytest.raises(Exception, match='each of the plane dims'):
        cm.cal_local_contour_lengths({'lat': 3})


def test_window_bounds():
    # odd: rolling(center=True) -- 2 nodes either side; even: one more node before the centre than after it
    lo, hi = LR.bounds(10, 5, 3)
    assert lo.tolist() == [0, 1, 4, 7] and hi.tolist() == [2, 5, 8, 9]
    lo, hi = LR.bounds(10, 4, 5)
    assert lo.tolist() == [0, 3] and hi.tolist() == [1, 6]
    lo, hi = LR.bounds(3, 8, 1)                                       # a plane smaller than the window
    assert lo.tolist() == [0, 0, 0] and hi.tolist() == [2, 2, 2]


def test_zonal_field_windows_closed_form():
    """q = f(row), unit Cartesian spacing: a level between two rows of the window is one straight line across it"""
    ny, nx, w, s = 40, 50, 9, 4
    q = np.repeat((np.arange(ny, dtype=np.float64) ** 1.5)[:, None], nx, axis=1)
    y, x = np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64)
    lv = LR.window_levels(q, (w, w), (s, s), min_periods=1)
    tot, cnt = LR.local_contour_lengths(q, lv, y, x, (w, w), (s, s))
    c0, c1 = LR.bounds(nx, w, s)
    r0, r1 = LR.bounds(ny, w, s)
    width = (c1 - c0).astype(np.float64)
    assert width[3] == w - 1 and width[0] == w // 2                   # interior: wx - 1; clipped: the clipped width
    # the mean of a window lies strictly between its first and last row's values: one line, the window's (clipped) width
    assert np.array_equal(tot, np.repeat(width[None, :], r0.size, axis=0))
    assert np.array_equal(cnt, np.repeat((c1 - c0)[None, :], r0.size, axis=0))
    # a given level: crossed only by the windows that hold it -- elsewhere NaN, 0 segments
    c = 20.3 ** 1.5
    tot, cnt = LR.local_contour_lengths(q, c, y, x, (w, w), (s, s))
    holds = (r0 <= 20) & (r1 >= 21)
    assert holds.any() and not holds.all()
    assert np.array_equal(tot[holds], np.repeat(width[None, :], holds.sum(), axis=0))
    assert np.isnan(tot[~holds]).all() and (cnt[~holds] == 0).all()


def test_min_periods_and_nan_levels():
    q = np.arange(30.0).reshape(5, 6)
    q[0, 0] = np.nan
    full = LR.window_levels(q, (3, 3), (2, 2))                        # min_periods = 9: clipped windows and the NaN's window miss it
    assert np.isnan(full[0]).all() and np.isnan(full[:, 0]).all() and not np.isnan(full[1, 1])
    some = LR.window_levels(q, (3, 3), (2, 2), min_periods=3)
    assert some[0, 0] == (1.0 + 6.0 + 7.0) / 3.0
    t, n = LR.local_contour_lengths(q, full, np.arange(5.0), np.arange(6.0), (3, 3), (2, 2))
    assert np.isnan(t[0]).all() and (n[0] == 0).all() and t[1, 1] > 0


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_sequential_mean_close_to_fsum(seed):
    rng = np.random.default_rng(seed)
    win = rng.standard_normal((101, 101)) * 10.0 ** rng.integers(-3, 4)
    win[rng.random(win.shape) < 0.08] = np.nan
    ok = ~np.isnan(win)
    n = int(ok.sum())
    exact = math.fsum(win[ok]) / n
    got = LR.sequential_mean(win, 1)
    assert abs(got - exact) <= n * 2.0 ** -52 * np.abs(win[ok]).max()
    assert np.isnan(LR.sequential_mean(win, n + 1)) and LR.sequential_mean(win, n) == got


def test_window_length_is_the_cropped_plane():
    rng = np.random.default_rng(4)
    q = rng.standard_normal((23, 31))
    y, x = CR.hashed_coords(23, 3, 5.0, 7.0), CR.hashed_coords(31, 4, -3.0, 2.0)
    t, n = LR.window_length(q, 0.1, y, x, (7, 6), (5, 4), 2, 3)
    rt, rn = CR.contour_lengths(q[7:14, 9:15], [0.1], y[7:14], x[9:15])
    assert (t, n) == (rt[0], rn[0]) and n > 0
