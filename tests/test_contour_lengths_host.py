"""Contour2D.cal_contour_lengths without a GPU: the entry points exist, and the numpy restatement of the rule (clength_ref)
meets closed forms, contourpy and the saddle pairing the kernel is pinned against."""
import math

import numpy as np
import pytest

import clength_ref as CR
import xcontour_amd as xa
from xcontour_amd import _native as nat


def test_entry_points_exist():
    assert callable(getattr(xa.Contour2D, 'cal_contour_lengths', None))
    assert callable(getattr(nat.Context, 'contour_lengths', None))
    for name in ('xc_contour_lengths', 'xc_contour_lengths_dev'):
        assert name in nat.PROTOTYPES


def test_facade_rejects_plane_without_coordinates():
    q = xa.DataArray(np.zeros((4, 6)), ('lat', 'lon'), {'lat': np.arange(4.)}, 'q')
    cm = xa.Contour2D(q, np.ones(4), {'X': 'lon', 'Y': 'lat'}, {'Y': 'lat'})
    with pytest.raises(Exception, match='coordinate values for the plane dim lon'):
        cm.cal_contour_lengths(np.array([0.5]))


def _hav(lat, dlon):
    return 2.0 * math.asin(math.sqrt(math.cos(lat) ** 2 * math.sin(dlon / 2) ** 2))


def test_zonal_field_latlon_closed_form():
    lat = np.linspace(-80.0, 80.0, 17)
    lon = np.arange(0.0, 360.0, 7.5)
    y, x = CR.plane_coords(lat, lon, True)
    q = np.repeat(np.arange(17.0)[:, None] * 3.0, lon.size, axis=1)           # q = f(row), increasing
    levels = np.array([0.7, 10.1, 25.5, 47.9])
    tot, cnt = CR.contour_lengths(q, levels, y, x, latlon=True)
    dlon = np.diff(x)                                                          # float32 radians: not exactly uniform
    for k, c in enumerate(levels):
        r = int(c // 3.0)
        fr = (c - q[r, 0]) / (q[r + 1, 0] - q[r, 0])
        yy = (y[r + 1] - y[r]) * fr + y[r]
        assert cnt[k] == lon.size - 1
        assert tot[k] == pytest.approx(math.fsum(_hav(yy, d) for d in dlon) * CR.RADIUS, rel=1e-12)


def test_cartesian_straight_lines_closed_form():
    ny, nx = 13, 21
    ycoord, xcoord = np.linspace(0.0, 600.0, ny), np.linspace(0.0, 2000.0, nx)
    col = np.repeat(np.arange(nx, dtype=np.float64)[None, :], ny, axis=0)
    tot, cnt = CR.contour_lengths(col, [3.25, 17.5], ycoord, xcoord)             # vertical lines
    assert np.array_equal(cnt, [ny - 1, ny - 1])
    assert np.allclose(tot, 600.0, rtol=1e-12, atol=0)
    diag = np.arange(ny, dtype=np.float64)[:, None] + np.arange(nx)[None, :]    # x + y = c on unit spacing
    yi, xi = np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64)
    for c in (2.5, 10.3, 25.7):
        t, _ = CR.contour_lengths(diag, [c], yi, xi)
        y0, y1 = max(0.0, c - (nx - 1)), min(ny - 1.0, c)
        assert t[0] == pytest.approx(math.sqrt(2.0) * (y1 - y0), rel=1e-12)


def test_levels_off_range_and_at_extrema_are_nan():
    q = np.add.outer(np.arange(5.0), np.arange(6.0))
    tot, cnt = CR.contour_lengths(q, [-1.0, 0.0, 9.0, 12.0, np.nan], np.arange(5.0), np.arange(6.0))
    assert np.isnan(tot).all() and cnt.sum() == 0


def _bumps(ny=61, nx=83):
    y, x = np.linspace(-3.0, 3.0, ny), np.linspace(-4.0, 4.5, nx)
    X, Y = np.meshgrid(x, y)
    z = np.exp(-((X - 1.0) ** 2 + (Y + 0.5) ** 2)) + 0.7 * np.exp(-((X + 1.5) ** 2 / 0.5 + (Y - 1.0) ** 2 / 2.0))
    return z, y, x


def test_restatement_matches_contourpy_on_gaussian_bumps():
    contourpy = pytest.importorskip('contourpy')
    z, y, x = _bumps()
    gen = contourpy.contour_generator(x, y, z, line_type='Separate')
    levels = [0.0537, 0.2113, 0.4471, 0.6389, 0.8123]
    tot, cnt = CR.contour_lengths(z, levels, y, x)
    for k, c in enumerate(levels):
        assert not np.any(z == c)
        lines = gen.lines(c)
        ref = sum(float(np.sum(np.hypot(*np.diff(l, axis=0).T))) for l in lines)
        nseg = sum(len(l) - 1 for l in lines)
        assert cnt[k] == nseg
        assert tot[k] == pytest.approx(ref, rel=1e-12)


@pytest.mark.parametrize('vals,low,high', [
    # case 9 (ul, lr above 0.5): low pairs (top, left) + (bottom, right)
    ((1.0, 0.0, 0.0, 3.0), math.hypot(0.5, 0.5) + math.hypot(5 / 6, 5 / 6), 2 * math.hypot(1 / 6, 0.5)),
    # case 6 (ur, ll above 0.5): low pairs (right, top) + (left, bottom)
    ((0.0, 1.0, 3.0, 0.0), math.hypot(0.5, 0.5) + math.hypot(5 / 6, 5 / 6), math.hypot(1 / 6, 0.5) + math.hypot(1 / 6, 0.5)),
])
def test_saddle_cells_pair_low(vals, low, high):
    ul, ur, ll, lr = vals
    q = np.array([[ul, ur], [ll, lr]])
    idx = np.arange(2.0)
    t, n = CR.contour_lengths(q, [0.5], idx, idx)
    th, _ = CR.contour_lengths(q, [0.5], idx, idx, pairs=CR.PAIRS_HIGH)
    assert n[0] == 2
    assert t[0] == pytest.approx(low, rel=1e-14) and th[0] == pytest.approx(high, rel=1e-14)
    assert abs(low - high) > 0.1


def test_level_on_node_values_drops_degenerate_and_keeps_duplicates():
    # row 1 equals the level with larger values on both sides: the cells above (case 3) and below (case 12) both emit the
    # shared side, 2 + 2 segments of length 1
    q = np.array([[2.0, 2.0, 2.0], [1.0, 1.0, 1.0], [2.0, 2.0, 2.0]])
    t, n = CR.contour_lengths(q, [1.0], np.arange(3.0), np.arange(3.0))
    assert n[0] == 4 and t[0] == 4.0
    # case 13 with ur on the level: top and right both sit on that corner, the segment is degenerate and dropped
    q = np.array([[1.0, 0.0], [1.0, 1.0]])
    t, n = CR.contour_lengths(q, [0.0], np.arange(2.0), np.arange(2.0))
    assert n[0] == 0 and np.isnan(t[0])


def _inputs(kind, ny=23, nx=31, seed=0):
    rng = np.random.default_rng(seed)
    if kind == 'saddle':
        q = np.indices((ny, nx)).sum(0) % 2 * 2.0 - 1.0 + 0.3 * rng.standard_normal((ny, nx))
    elif kind == 'node':
        q = rng.integers(0, 6, size=(ny, nx)).astype(np.float64)
    else:
        q = rng.standard_normal((ny, nx))
    if kind == 'nan':
        q[rng.random(q.shape) < 0.08] = np.nan
    levels = {'node': np.array([-1.0, 0.0, 1.0, 2.0, 2.0, 2.5, 3.0, 5.0, 6.0])}.get(kind, np.linspace(-2.0, 2.0, 17))
    return q, levels


@pytest.mark.parametrize('latlon', [False, True])
@pytest.mark.parametrize('kind', ['random', 'saddle', 'nan', 'node'])
def test_fast_restatement_equals_the_level_loop(kind, latlon):
    """segments_fast / contour_lengths_fast emit the per-level loop's segments: the same end points and the same lengths, bit for
    bit, level by level (in another order); counts equal, totals to rounding.  Coordinates that differ in every cell, latitude
    descending on the sphere."""
    q, levels = _inputs(kind, seed=len(kind))
    ny, nx = q.shape
    if latlon:
        y = np.deg2rad(CR.hashed_coords(ny, 1, -80.0, 160.0 / ny, descending=True))
        x = np.deg2rad(CR.hashed_coords(nx, 2, 0.0, 300.0 / nx))
    else:
        y, x = CR.hashed_coords(ny, 3, 5.0, 7.0), CR.hashed_coords(nx, 4, -3.0, 2.0)
    lv = levels[::-1].copy() if kind == 'random' else levels               # any order
    k, r1, c1, r2, c2, ln = CR.segments_fast(q, lv, y, x, latlon)
    tot, cnt = CR.contour_lengths_fast(q, lv, y, x, latlon)
    rt, rn = CR.contour_lengths(q, lv, y, x, latlon)
    assert np.array_equal(cnt, rn) and cnt.sum() > 0
    assert np.array_equal(np.isnan(tot), np.isnan(rt))
    ok = ~np.isnan(rt)
    assert np.all(np.abs(tot[ok] - rt[ok]) <= 1e-13 * np.abs(rt[ok]))
    for j, c in enumerate(lv):
        m = k == j
        a, b, e, d = CR.segments(q, c)
        want = sorted(zip(a, b, e, d, CR.segment_lengths(q, c, y, x, latlon)))
        got = sorted(zip(r1[m], c1[m], r2[m], c2[m], ln[m]))
        assert np.array_equal(np.array(got).view(np.int64), np.array(want).view(np.int64)) if want else not got, (kind, j)


def test_fast_restatement_small_chunks_and_empty_planes():
    q, lv = _inputs('saddle', 9, 12)
    y, x = np.arange(9.0), CR.hashed_coords(12)
    a = CR.segments_fast(q, lv, y, x)
    b = CR.segments_fast(q, lv, y, x, chunk=7)
    assert a[0].size > 100 and sorted(zip(*a)) == sorted(zip(*b))
    for shape in ((1, 12), (9, 1)):
        t, n = CR.contour_lengths_fast(np.zeros(shape), [0.5, 1.0], np.arange(shape[0] * 1.0), np.arange(shape[1] * 1.0))
        assert np.isnan(t).all() and (n == 0).all()


def test_det_totals_exact_where_the_window_holds_every_bit():
    """a tracer varying along x only: every segment is vertical, |y[r+1] - y[r]|; with spacings of 20 significant bits the
    fixed-point sum is the exact sum, so det_totals is math.fsum bit for bit"""
    ny, nx = 40, 9
    dy = np.floor(np.diff(CR.hashed_coords(ny, 5)) * 2 ** 12) / 2 ** 12
    y = np.concatenate([[0.0], np.cumsum(dy)])
    x = CR.hashed_coords(nx, 6)
    q = np.repeat(np.arange(nx, dtype=np.float64)[None, :], ny, axis=0)
    lv = np.array([0.5, 3.25, 7.75, 8.0, 9.0])
    t = CR.det_totals(q, lv, y, x)
    exact = math.fsum(dy)
    assert [t[0], t[1], t[2]] == [exact] * 3 and np.isnan(t[3:]).all()
    tl = CR.det_totals(q, lv, y * 0.01, x * 0.01, latlon=True)
    assert tl[0] == tl[1] == tl[2] and abs(tl[0] / (0.01 * exact * CR.RADIUS) - 1.0) < 1e-12


def test_det_totals_drops_what_falls_under_the_window():
    """one very wide column lifts the window: segments 2^-150 of it lose their low chunk (and the shortest all of it), the model
    follows the chunk rule of the oracle, not the exact sum"""
    import xcontour_oracle as O
    ny = 3
    y = np.array([0.0, 3 * 2.0 ** -140, 3 * 2.0 ** -140 + 2.0 ** -160])                 # the window ends at 2^-139
    x = np.array([0.0, 2.0 ** 40, 2.0 ** 40 + 1.0])
    q = np.repeat(np.array([[0.0, 1.0, 2.0]]), ny, axis=0)
    lv = np.array([1.5])
    t = CR.det_totals(q, lv, y, x)
    top = O.det_window_top(CR.clen_bound(y, x, False))
    want = sum(O.det_chunks(w, top, 4) for w in np.diff(y))
    assert t[0] == math.ldexp(float(want), top - 48 * 4)
    assert t[0] == 2.0 ** -139 and math.fsum(np.diff(y)) == 3 * 2.0 ** -140 + 2.0 ** -160
