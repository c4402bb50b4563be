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


# ------------------------------------------------------------------ the helpers of the GPU geometry tests
def test_sequential_mean_starts_from_zero():
    """the rule of xc_lclen.hip: every row and the total start from 0.0, so a sum is never -0.0"""
    for shape in ((1, 1), (1, 7), (5, 1), (4, 6)):
        z = np.full(shape, -0.0)
        assert math.copysign(1.0, np.cumsum(z.ravel())[-1]) == -1.0               # (a bare cumsum starts from its first element)
        m = LR.sequential_mean(z, 1)
        assert m == 0.0 and math.copysign(1.0, m) == 1.0, shape
    z = np.full((4, 6), -0.0)
    z[0, 0] = z[2, 3] = z[3, 5] = np.nan
    m = LR.sequential_mean(z, 1)
    assert m == 0.0 and math.copysign(1.0, m) == 1.0
    z[:] = np.nan                                                                 # 0 / 0: NaN, whatever min_periods = 0 lets through
    assert np.isnan(LR.sequential_mean(z, 0)) and np.isnan(LR.sequential_mean(z, 1))
    lv = LR.window_levels(np.full((6, 7), -0.0), (3, 3), (2, 2), 1)
    assert (lv == 0.0).all() and (np.copysign(1.0, lv) == 1.0).all()
    # the order is still the kernel's: rows left to right, then the row sums top to bottom
    w = np.array([[1e16, 1.0, -1e16], [1.0, 1.0, 1.0]])
    assert LR.sequential_mean(w, 1) == ((1e16 + 1.0 - 1e16) + (1.0 + 1.0 + 1.0)) / 6.0


# (window, plane, clipped rows, clipped columns) -> (threads, mean rounds, strips, carry rounds): the shapes test_gpu_lclen_geometry walks
LAUNCH_TABLE = [
    ((2, 2049), (6, 2100), 2, 2049, (64, 1, 32, 2)),         # 2048 cells exactly: one wave, 31 + 1 strips
    ((2, 2050), (6, 2100), 2, 2050, (256, 1, 33, 1)),        # one cell more: four waves
    ((2, 2049), (6, 2100), 1, 2049, (64, 1, 0, 0)),          # clipped to one node row: no cells
    ((2, 2049), (6, 2100), 2, 1025, (64, 1, 16, 1)),         # clipped in X: the threads stay the unclipped window's
    ((150, 5), (200, 9), 150, 5, (64, 3, 10, 1)),
    ((150, 5), (200, 9), 129, 5, (64, 3, 8, 1)),
    ((150, 5), (200, 9), 128, 5, (64, 2, 8, 1)),
    ((150, 5), (200, 9), 75, 3, (64, 2, 5, 1)),
    ((128, 5), (200, 9), 65, 5, (64, 2, 4, 1)),
    ((128, 5), (200, 9), 64, 5, (64, 1, 4, 1)),
    ((300, 12), (330, 14), 300, 12, (256, 2, 19, 1)),
    ((300, 12), (330, 14), 257, 12, (256, 2, 16, 1)),
    ((300, 12), (330, 14), 256, 12, (256, 1, 16, 1)),
    ((300, 12), (330, 14), 150, 6, (256, 1, 10, 1)),
    ((65, 1985), (70, 2100), 65, 1985, (256, 1, 124, 1)),    # 31 full strips in each of the four waves
    ((65, 1986), (70, 2100), 65, 1986, (256, 1, 128, 2)),
    ((81, 1985), (70, 2100), 70, 1985, (256, 1, 155, 2)),    # taller than the plane: 69 cell rows
    ((16, 64), (40, 300), 16, 64, (64, 1, 1, 1)),
    ((17, 65), (40, 300), 17, 65, (64, 1, 1, 1)),
    ((18, 66), (40, 300), 18, 66, (64, 1, 4, 1)),
    ((16, 130), (40, 300), 16, 130, (64, 1, 3, 1)),
    ((17, 129), (40, 300), 17, 129, (64, 1, 2, 1)),          # 16 x 128 = 2048
    ((17, 130), (40, 300), 17, 130, (256, 1, 3, 1)),         # 16 x 129 = 2064
    ((18, 129), (40, 300), 18, 129, (256, 1, 4, 1)),
    ((18, 130), (40, 300), 18, 130, (256, 1, 6, 1)),
    ((33, 65), (40, 70), 33, 65, (64, 1, 2, 1)),
    ((35, 65), (40, 70), 33, 65, (256, 1, 2, 1)),            # the same nodes after clipping, the other block size
    ((1200, 1400), (600, 700), 600, 700, (256, 3, 418, 4)),
    ((12, 9), (7, 5), 7, 5, (64, 1, 1, 1)),                  # a plane smaller than the window
]


@pytest.mark.parametrize('window,plane,rows,cols,want', LAUNCH_TABLE)
def test_launch_shape_table(window, plane, rows, cols, want):
    assert LR.launch_shape(window, plane, rows, cols) == want


def _x_only_plane(ny, nx, seed):
    """a field that varies along x only on few-bit coordinates: every segment is one y spacing, exactly"""
    rng = np.random.default_rng(seed)
    q = np.broadcast_to(rng.uniform(-3.0, 3.0, nx)[None, :], (ny, nx)).copy()
    return q, CR.few_bits(ny, 1, 1.0), CR.few_bits(nx, 2, 1.0)


def test_det_window_total_is_fsum_on_few_bit_coordinates():
    ny, nx = 40, 150
    q, y, x = _x_only_plane(ny, nx, 3)
    window, stride = (17, 70), (9, 40)
    (r0, r1), (c0, c1) = LR.bounds(ny, 17, 9), LR.bounds(nx, 70, 40)
    n = 0
    for wj in range(r0.size):
        for wi in range(c0.size):
            sub = q[r0[wj]:r1[wj] + 1, c0[wi]:c1[wi] + 1]
            _, _, _, _, _, ln = CR.segments_fast(sub, [0.2], y[r0[wj]:r1[wj] + 1], x[c0[wi]:c1[wi] + 1])
            assert ln.size > 20 and set(ln.tolist()) <= set(np.diff(y).tolist())     # the premise: whole y spacings
            got = LR.det_window_total(q, 0.2, y, x, window, stride, wj, wi)
            want = math.fsum(ln)
            assert np.float64(got).view(np.int64) == np.float64(want).view(np.int64), (wj, wi)
            n += 1
    assert n == 20
    assert np.isnan(LR.det_window_total(q, np.nan, y, x, window, stride, 1, 1))
    assert np.isnan(LR.det_window_total(q, 99.0, y, x, window, stride, 1, 1))          # no segment: a total of 0 is NaN


def test_det_window_total_takes_the_bound_of_the_whole_plane():
    """a cell 2^120 times the others that the window does not own lifts the window top: the window's short segments lose their low
    bits -- the crop's own bound would keep them"""
    ny, nx = 40, 150
    q, _, x = _x_only_plane(ny, nx, 3)
    y = CR.few_bits(ny, 1, 2.0 ** -44)
    window, stride, at = (17, 70), (9, 40), (2, 1)                     # window (2, 1): rows 10..26, columns 5..74
    plain = LR.det_window_total(q, 0.2, y, x, window, stride, *at)
    _, _, _, _, _, ln = CR.segments_fast(q[10:27, 5:75], [0.2], y[10:27], x[5:75])
    assert plain == math.fsum(ln)
    xw = x.copy()
    xw[100:] += 2.0 ** 120                                             # the cell between columns 99 and 100
    wide = LR.det_window_total(q, 0.2, y, xw, window, stride, *at)
    assert np.array_equal(xw[5:75], x[5:75]) and wide != plain and 0 < plain - wide < 1e-3 * plain
