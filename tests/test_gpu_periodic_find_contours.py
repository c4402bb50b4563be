"""Contour2D.find_contours(periodic=...) / xc.find_contour(periodic=...) on the GPU against the restatement
contour_join_periodic_ref (vertices bit for bit, the same closed flags and winding numbers, the same order of polylines), against
periodic K10's totals, and on the barotropic field's circumpolar rings."""
import numpy as np
import pytest

import clength_ref as CR
import contour_join_periodic_ref as PJ
import contour_join_ref as JR
import xcontour_amd as xa

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def facade(q, y, x, lead=(), transposed=False):
    dims = tuple('d%d' % i for i in range(len(lead))) + ('latitude', 'longitude')
    c = {'latitude': y, 'longitude': x}
    c.update({'d%d' % i: np.arange(n) for i, n in enumerate(lead)})
    if transposed:
        tr = xa.DataArray(np.ascontiguousarray(np.swapaxes(q, -1, -2)), dims[:-2] + ('longitude', 'latitude'), c, 'q')
    else:
        tr = xa.DataArray(q, dims, c, 'q')
    return xa.Contour2D(tr, np.ones(len(y)), {'X': 'longitude', 'Y': 'latitude'}, {'Y': 'latitude'}, dtype=np.float64), tr


def same_polylines(got, ref, what=''):
    """one slab: (polylines[k], closed[k], winding[k]) against the restatement's"""
    (gp, gc, gw), (rp, rc, rw) = got, ref
    assert len(gp) == len(rp), what
    for k in range(len(rp)):
        assert len(gp[k]) == len(rp[k]), '%s level %d: %d polylines, restatement %d' % (what, k, len(gp[k]), len(rp[k]))
        assert list(gc[k]) == list(rc[k]), '%s level %d: closed flags' % (what, k)
        assert list(gw[k]) == list(rw[k]), '%s level %d: winding numbers' % (what, k)
        for a, b in zip(gp[k], rp[k]):
            assert a.dtype == np.float64 and a.shape == b.shape and np.array_equal(bits(a), bits(b)), '%s level %d' % (what, k)


def both(cm, lv, periodic, **kw):
    return cm.find_contours(lv, periodic=periodic, return_closed=True, return_winding=True, **kw)


@pytest.fixture(scope='module')
def baro_levels(baro):
    q = baro[0].astype(np.float64)
    return np.linspace(q.min(), q.max(), 9)[1:-1]


@pytest.fixture(scope='module')
def baro_ref(baro, baro_levels):
    """the restatement of the barotropic field at the 7 interior levels: index space, and on the coordinates with 360 degrees"""
    q, lat, lon = baro
    q = q.astype(np.float64)
    return PJ.polylines(q, baro_levels), PJ.polylines(q, baro_levels, lat, lon, 360.0)


@pytest.mark.parametrize('transposed', [False, True])
def test_barotropic_field(baro, baro_levels, baro_ref, transposed):
    q, lat, lon = baro
    cm, _ = facade(q, lat, lon, transposed=transposed)
    same_polylines(both(cm, baro_levels, True, index=True), baro_ref[0], 'index')
    got = both(cm, baro_levels, True)
    same_polylines(got, baro_ref[1], 'periodic=True')
    same_polylines(both(cm, baro_levels, 360.0), baro_ref[1], 'periodic=360.0')
    # every level: rings only, exactly one of them round the globe, its last vertex the first one period on
    polys, closed, wind = got
    for k in range(baro_levels.size):
        assert all(closed[k]) and sorted(abs(w) for w in wind[k])[-2:] in ([1], [0, 1])
        (i,) = [i for i, w in enumerate(wind[k]) if w != 0]
        p, w = polys[k][i], wind[k][i]
        assert p[-1, 0] == p[0, 0] and p[-1, 1] == p[0, 1] + w * 360.0
    # the flags alone, the winding numbers alone, neither
    assert cm.find_contours(baro_levels, periodic=True, return_winding=True)[1] == wind
    assert cm.find_contours(baro_levels, periodic=True, return_closed=True)[1] == closed
    assert len(cm.find_contours(baro_levels, periodic=True)) == baro_levels.size


def test_descending_longitude(baro, baro_levels):
    q, lat, lon = baro
    qd, lond = np.ascontiguousarray(q[:, ::-1]), lon[::-1].copy()
    cm, _ = facade(qd, lat, lond)
    ref = PJ.polylines(qd.astype(np.float64), baro_levels, lat, lond, -360.0)
    same_polylines(both(cm, baro_levels, True), ref, 'periodic=True')
    same_polylines(both(cm, baro_levels, -360.0), ref, 'periodic=-360.0')
    assert sum(abs(w) for row in ref[2] for w in row) == baro_levels.size
    with pytest.raises(Exception, match='runs against the X coordinate'):
        cm.find_contours(baro_levels, periodic=360.0)


def test_nan_mask_and_nonuniform_coordinates():
    rng = np.random.default_rng(21)
    ny, nx = 61, 140
    y0, x0 = np.meshgrid(np.linspace(-1.4, 1.4, ny), np.arange(nx) * (2.0 * np.pi / nx), indexing='ij')
    q = 2.0 * np.sin(y0) + 0.4 * np.cos(3 * x0) * np.cos(y0) ** 2 + 0.05 * rng.standard_normal((ny, nx))
    q[20:28, 30:50] = np.nan
    q[40:44, [0, 1, nx - 1]] = np.nan                       # a hole across the seam
    q[rng.random(q.shape) < 0.01] = np.nan
    lv = np.linspace(-1.8, 1.8, 9)
    for y, x, P in ((CR.hashed_coords(ny, 1, -40.0, 1.3), CR.hashed_coords(nx, 2, 10.0, 2.5), 371.25),
                    (CR.hashed_coords(ny, 3, -40.0, 1.3, descending=True), np.linspace(0.0, 357.5, nx), True)):
        assert abs(x[-1] - x[0]) < 360.0
        cm, _ = facade(q, y, x)
        got = both(cm, lv, P)
        same_polylines(got, PJ.polylines(q, lv, y, x, 360.0 if P is True else P), 'coordinates')
        gi = both(cm, lv, P, index=True)
        same_polylines(gi, PJ.polylines(q, lv), 'index')
        # open polylines beside the NaN cells, and polylines that run through the seam cell and on past it
        assert any(not c for row in got[1] for c in row) and any(p[:, 1].max() > nx for row in gi[0] for p in row)


def test_leading_dims_unsorted_levels_and_a_nan_level():
    rng = np.random.default_rng(22)
    q = (rng.standard_normal((2, 3, 25, 40)) + 0.5 * np.arange(25)[:, None]).astype(np.float32)
    y, x = np.linspace(0.0, 48.0, 25), np.linspace(0.0, 78.0, 40)
    cm, _ = facade(q, y, x, lead=(2, 3))
    lv = np.array([6.5, 1.0, np.nan, 9.5, 3.0, 99.0])
    got = both(cm, lv, 80.0)
    assert all(len(g) == 6 and all(len(s) == 6 for s in g) for g in got)
    for s in range(6):
        ref = PJ.polylines(q.reshape(6, 25, 40)[s].astype(np.float64), lv, y, x, 80.0)
        same_polylines(tuple(g[s] for g in got), ref, 'slab %d' % s)
        assert got[0][s][2] == [] and got[0][s][5] == [] and len(got[0][s][0]) > 0
    assert any(w != 0 for s in got[2] for row in s for w in row)
    # levels labelled per slab, index space (no coordinates needed for the period: only its truth value matters)
    per = np.sort(rng.uniform(2.0, 10.0, (2, 3, 4)), axis=-1)
    ctr = xa.DataArray(per, ('d0', 'd1', 'contour'), {'d0': np.arange(2), 'd1': np.arange(3), 'contour': np.arange(4.0)}, 'q')
    for P in (True, 5.0):
        got = both(cm, ctr, P, index=True)
        for s in range(6):
            ref = PJ.polylines(q.reshape(6, 25, 40)[s].astype(np.float64), per.reshape(6, 4)[s])
            same_polylines(tuple(g[s] for g in got), ref, 'per-slab levels, slab %d' % s)


def test_consistent_with_periodic_contour_lengths():
    """Cartesian lengths on coordinates and a period float32 holds exactly (cal_contour_lengths casts them to float32; with
    latlon=True it also rounds the radians to float32, which find_contours -- float64 throughout -- does not): the pieces of a
    level add up to periodic K10's total within 1e-12 relative, K10's own bar against its restatement, and a level has no pieces
    exactly where K10 returns NaN"""
    rng = np.random.default_rng(23)
    ny, nx = 97, 301
    q = rng.standard_normal((ny, nx)) + 0.08 * np.arange(ny)[:, None]
    q[rng.random(q.shape) < 0.03] = np.nan
    y, x = np.arange(ny) * 0.75 - 30.0, np.arange(nx) * 1.25
    P = nx * 1.25 + 0.5
    assert np.array_equal(y.astype(np.float32), y) and np.array_equal(x.astype(np.float32), x) and float(np.float32(P)) == P
    cm, _ = facade(q, y, x)
    lv = np.concatenate([[-9.0], np.linspace(-1.0, 8.0, 9), [float(np.nanmax(q)), 21.0]])
    lens = cm.cal_contour_lengths(lv, periodic=P).values
    plain = cm.cal_contour_lengths(lv).values
    got = cm.find_contours(lv, periodic=P)
    assert np.isnan(lens[[0, -2, -1]]).all() and (lens[1:-2] > plain[1:-2]).all()
    for k in range(lv.size):
        if np.isnan(lens[k]):
            assert got[k] == []
        else:
            t = sum(xa.polyline_length(p) for p in got[k])
            assert len(got[k]) > 0 and abs(t - lens[k]) <= 1e-12 * lens[k], (k, t, lens[k])


def test_without_periodic_nothing_changes(baro, baro_levels):
    q, lat, lon = baro
    cm, _ = facade(q, lat, lon)
    ref, rc = JR.polylines(q.astype(np.float64), baro_levels, lat, lon)
    zeros = [[0] * len(c) for c in rc]
    for kw in (dict(), dict(periodic=False), dict(periodic=None)):
        same_polylines(cm.find_contours(baro_levels, return_closed=True, return_winding=True, **kw), (ref, rc, zeros), str(kw))
    ri, rci = JR.polylines(q.astype(np.float64), baro_levels)
    same_polylines(cm.find_contours(baro_levels, index=True, return_closed=True, return_winding=True, periodic=False), (ri, rci, zeros), 'index')
    out = cm.find_contours(baro_levels)
    assert isinstance(out, list) and len(out) == baro_levels.size and isinstance(out[0], list)
    two = cm.find_contours(baro_levels, return_closed=True)
    assert isinstance(two, tuple) and len(two) == 2 and two[1] == rc


def test_module_level_find_contour_periodic(baro):
    q, lat, lon = baro
    cm, tr = facade(q, lat, lon)
    level = float(np.median(q))
    want = cm.find_contours([level], periodic=True)[0]
    for P in (True, 360.0):
        got = xa.find_contour(tr, ['latitude', 'longitude'], level, periodic=P)
        assert len(got) == len(want) > 0
        for a, b in zip(got, want):
            assert np.array_equal(bits(a), bits(b))
    plain = xa.find_contour(tr, ['latitude', 'longitude'], level)
    assert sum(len(p) for p in want) > sum(len(p) for p in plain)                    # the seam cell's vertices
    with pytest.raises(NotImplementedError, match='not supported yet'):
        xa.find_contour(tr, ['latitude', 'longitude'], level, period=[None, 360.0])
    with pytest.raises(NotImplementedError, match='not supported yet'):
        xa.find_contour(tr, ['latitude', 'longitude'], level, period=[None, 360.0], periodic=True)
