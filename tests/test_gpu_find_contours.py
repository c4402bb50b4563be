"""Contour2D.find_contours / xc.find_contour on the GPU against the restatement contour_join_ref (vertices bit for bit, the same
closed flags, the same order of polylines), against K10's totals, and against closed forms."""
import os

import numpy as np
import pytest

import clength_ref as CR
import contour_join_ref as JR
import xcontour_amd as xa

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def facade(q, y, x, lead=()):
    dims = tuple('d%d' % i for i in range(len(lead))) + ('latitude', 'longitude')
    c = {'latitude': y, 'longitude': x}
    c.update({'d%d' % i: np.arange(n) for i, n in enumerate(lead)})
    tr = xa.DataArray(q, dims, c, 'q')
    return xa.Contour2D(tr, np.ones(len(y)), {'X': 'longitude', 'Y': 'latitude'}, {'Y': 'latitude'}, dtype=np.float64), tr


def same_polylines(got, closed, ref, ref_closed, what=''):
    """one slab: got[k] / ref[k] lists of (n, 2) arrays"""
    assert len(got) == len(ref), what
    for k in range(len(ref)):
        assert len(got[k]) == len(ref[k]), '%s level %d: %d polylines, restatement %d' % (what, k, len(got[k]), len(ref[k]))
        assert list(closed[k]) == list(ref_closed[k]), '%s level %d: closed flags' % (what, k)
        for a, b in zip(got[k], ref[k]):
            assert a.dtype == np.float64 and a.shape == b.shape and np.array_equal(bits(a), bits(b)), '%s level %d' % (what, k)


def test_barotropic_field(baro):
    q, lat, lon = baro
    cm, _ = facade(q, lat, lon)
    lv = np.linspace(float(q.min()), float(q.max()), 21)
    for index in (True, False):
        got, closed = cm.find_contours(lv, index=index, return_closed=True)
        ref, rc = JR.polylines(q.astype(np.float64), lv, *((None, None) if index else (lat, lon)))
        same_polylines(got, closed, ref, rc, 'index=%s' % index)
    assert sum(len(p) for p in got) > 20 and any(any(c) for c in closed) and any(not all(c) for c in closed)
    assert cm.find_contours(lv) is not None and len(cm.find_contours(lv)) == 21       # without the flags: the lists alone


def test_nan_mask_nonuniform_and_descending_coordinates():
    rng = np.random.default_rng(21)
    ny, nx = 61, 140
    y0, x0 = np.meshgrid(np.linspace(-1.4, 1.4, ny), np.linspace(0.0, 6.0, nx), indexing='ij')
    q = 2.0 * np.sin(y0) + 0.4 * np.cos(3 * x0) * np.cos(y0) ** 2 + 0.05 * rng.standard_normal((ny, nx))
    q[20:28, 30:50] = np.nan
    q[rng.random(q.shape) < 0.01] = np.nan
    lv = np.linspace(-1.8, 1.8, 9)
    for y, x in ((CR.hashed_coords(ny, 1, -40.0, 1.3), CR.hashed_coords(nx, 2, 10.0, 2.5)),
                 (CR.hashed_coords(ny, 3, -40.0, 1.3, descending=True), np.linspace(0.0, 357.5, nx))):
        cm, _ = facade(q, y, x)
        got, closed = cm.find_contours(lv, return_closed=True)
        same_polylines(got, closed, *JR.polylines(q, lv, y, x), what='coordinates')
        gi, ci = cm.find_contours(lv, index=True, return_closed=True)
        same_polylines(gi, ci, *JR.polylines(q, lv), what='index')


def test_leading_dims_unsorted_levels_and_a_nan_level():
    rng = np.random.default_rng(22)
    q = rng.standard_normal((2, 3, 25, 40)).astype(np.float32)
    y, x = np.linspace(0.0, 48.0, 25), np.linspace(0.0, 78.0, 40)
    cm, _ = facade(q, y, x, lead=(2, 3))
    lv = np.array([0.5, -1.0, np.nan, 1.5, 0.0, 9.0])
    got, closed = cm.find_contours(lv, return_closed=True)
    assert len(got) == 6 and all(len(g) == 6 for g in got)
    for s in range(6):
        ref, rc = JR.polylines(q.reshape(6, 25, 40)[s].astype(np.float64), lv, y, x)
        same_polylines(got[s], closed[s], ref, rc, 'slab %d' % s)
        assert got[s][2] == [] and got[s][5] == [] and len(got[s][0]) > 0
    # levels labelled per slab
    per = np.sort(rng.uniform(-1.0, 1.0, (2, 3, 4)), axis=-1)
    ctr = xa.DataArray(per, ('d0', 'd1', 'contour'), {'d0': np.arange(2), 'd1': np.arange(3), 'contour': np.arange(4.0)}, 'q')
    got = cm.find_contours(ctr, index=True)
    for s in range(6):
        ref, _ = JR.polylines(q.reshape(6, 25, 40)[s].astype(np.float64), per.reshape(6, 4)[s])
        same_polylines(got[s], [[None] * len(g) for g in got[s]], ref, [[None] * len(r) for r in ref], 'per-slab levels, slab %d' % s)
    # an int goes through cal_contours
    n5 = cm.find_contours(5, index=True)
    lv5 = cm.cal_contours(5).values.reshape(6, 5)
    for s in range(6):
        ref, _ = JR.polylines(q.reshape(6, 25, 40)[s].astype(np.float64), lv5[s])
        assert [len(p) for p in n5[s]] == [len(p) for p in ref]


def test_consistent_with_contour_lengths():
    """Cartesian lengths on coordinates float32 holds exactly (cal_contour_lengths casts them to float32; with latlon=True it
    also rounds the radians to float32, which find_contours -- float64 throughout -- does not): the pieces of a level add up to
    K10's total within 1e-12 relative, K10's own bar against its restatement, and a level has no pieces exactly where K10
    returns NaN"""
    rng = np.random.default_rng(23)
    ny, nx = 97, 301
    q = rng.standard_normal((ny, nx))
    q[rng.random(q.shape) < 0.03] = np.nan
    y, x = np.arange(ny) * 0.75 - 30.0, np.arange(nx) * 1.25
    assert np.array_equal(y.astype(np.float32), y) and np.array_equal(x.astype(np.float32), x)
    cm, _ = facade(q, y, x)
    lv = np.concatenate([[-9.0], np.linspace(-2.0, 2.0, 9), [float(np.nanmax(q)), 11.0]])
    lens = cm.cal_contour_lengths(lv).values
    got = cm.find_contours(lv)
    assert np.isnan(lens[[0, -2, -1]]).all()
    for k in range(lv.size):
        if np.isnan(lens[k]):
            assert got[k] == []
        else:
            t = sum(xa.polyline_length(p) for p in got[k])
            assert len(got[k]) > 0 and abs(t - lens[k]) <= 1e-12 * lens[k], (k, t, lens[k])


def test_polyline_length_latlon_is_the_haversine():
    p = np.array([[10.0, 20.0], [10.5, 21.0], [12.0, 21.0]])
    y, x = np.deg2rad(p[:, 0]), np.deg2rad(p[:, 1])
    want = float(np.sum(CR.haversine(x[:-1], y[:-1], x[1:], y[1:])) * CR.RADIUS)
    assert xa.polyline_length(p, latlon=True) == want
    assert xa.polyline_length(p) == float(np.hypot(0.5, 1.0) + 1.5)
    assert xa.polyline_length(p[:1]) == 0.0


def test_closed_forms():
    ny, nx = 9, 23
    y, x = np.arange(ny) * 2.0, np.arange(nx) * 3.0
    rows = np.repeat(np.arange(ny, dtype=np.float64)[:, None], nx, axis=1)
    cm, _ = facade(rows, y, x)
    (line,), (cl,) = (v[0] for v in cm.find_contours([3.25], index=True, return_closed=True))
    assert cl is False and line.shape == (nx, 2)
    assert (line[:, 0] == 3.25).all() and sorted(line[:, 1].tolist()) == list(np.arange(nx, dtype=np.float64))
    (line,) = cm.find_contours([3.25])[0]
    assert (line[:, 0] == 6.5).all() and sorted(line[:, 1].tolist()) == list(x)
    # a cone: one ring, its first and last vertices equal, every vertex at the level's radius up to the linear interpolation
    n = 41
    yy, xx = np.meshgrid(np.arange(n) - 20.0, np.arange(n) - 20.0, indexing='ij')
    cone = -np.hypot(yy, xx)
    cm, _ = facade(cone, np.arange(n) * 1.0, np.arange(n) * 1.0)
    (ring,), (cl,) = (v[0] for v in cm.find_contours([-10.3], index=True, return_closed=True))
    assert cl is True and ring.shape[0] > 40 and np.array_equal(ring[0], ring[-1])
    r = np.hypot(ring[:, 0] - 20.0, ring[:, 1] - 20.0)
    assert np.abs(r - 10.3).max() < 0.05
    # a NaN hole on its rim opens it
    cone[20, 30] = np.nan
    cm, _ = facade(cone, np.arange(n) * 1.0, np.arange(n) * 1.0)
    (arc,), (cl,) = (v[0] for v in cm.find_contours([-10.3], index=True, return_closed=True))
    assert cl is False and not np.array_equal(arc[0], arc[-1]) and arc.shape[0] > 30


def test_module_level_find_contour(baro):
    q, lat, lon = baro
    cm, tr = facade(q, lat, lon)
    level = float(np.median(q))
    got = xa.find_contour(tr, ['latitude', 'longitude'], level)
    want = cm.find_contours([level])[0]
    assert len(got) == len(want) > 0
    for a, b in zip(got, want):
        assert np.array_equal(bits(a), bits(b))
    assert len(xa.find_contour(tr, ['latitude', 'longitude'], level, period=[None, None])) == len(want)
    with pytest.raises(NotImplementedError, match='not supported yet'):
        xa.find_contour(tr, ['latitude', 'longitude'], level, period=[None, 360.0])
