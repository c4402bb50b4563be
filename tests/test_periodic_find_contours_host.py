"""The periodic X direction of Contour2D.find_contours without a GPU: the host builder of vertices, laps and winding numbers
(xcontour_amd.contour_polylines) against the plain loop of the restatement contour_join_periodic_ref, bit for bit, on records
the restatement makes; what periodic tracing does to the barotropic field; the errors raised before any device work; and the
new entry points."""
import inspect

import numpy as np
import pytest

import contour_join_periodic_ref as PJ
import xcontour_amd as xa
from xcontour_amd import _native as nat

NEW = ('xc_contour_segments_periodic', 'xc_contour_segments_periodic_dev')


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def built(q, lv, y=None, x=None, period=None):
    """the records of the restatement, joined by xc_join_segments and built by the host function -> per level"""
    cnt, ef, et, pts = PJ.stack_records(q[None], lv)
    off = np.concatenate([[0], np.cumsum(cnt.ravel().astype(np.int64))])
    walk, poff, closed, rpo = nat.join_segments(off, ef, et)
    return xa.contour_polylines(walk, poff, closed, rpo, pts, nx=q.shape[1], ycoord=y, xcoord=x, period=period)


def same(got, ref, what=''):
    (gp, gc, gw), (rp, rc, rw) = got, ref
    assert len(gp) == len(rp) == len(gc) == len(gw), what
    for k in range(len(rp)):
        assert len(gp[k]) == len(rp[k]), '%s level %d: %d polylines, restatement %d' % (what, k, len(gp[k]), len(rp[k]))
        assert list(gc[k]) == list(rc[k]), '%s level %d: closed' % (what, k)
        assert list(gw[k]) == list(rw[k]) and all(type(w) is int for w in gw[k]), '%s level %d: winding' % (what, k)
        for a, b in zip(gp[k], rp[k]):
            assert a.dtype == np.float64 and a.shape == b.shape and np.array_equal(bits(a), bits(b)), '%s level %d' % (what, k)


def both_ways(q, lv, y, x, period, what):
    ref = PJ.polylines(q, lv)
    same(built(q, lv), ref, what + ' index')
    same(built(q, lv, y, x, period), PJ.polylines(q, lv, y, x, period), what + ' coordinates')
    return ref


def zonal(ny=9, nx=12):
    lat = np.arange(ny, dtype=np.float64)
    lon = np.arange(nx) * (2.0 * np.pi / nx)
    return lat[:, None] + 0.2 * np.sin(2.0 * lon)[None, :]


def test_wavy_zonal_field_one_ring_per_level_winding_once():
    q = zonal()
    ny, nx = q.shape
    lv = np.array([1.1, 3.1, 6.9])                       # each crosses a row four times: 12 + 4 segments
    y, x = np.linspace(-60.0, 60.0, ny), np.arange(nx) * 30.0
    polys, closed, wind = both_ways(q, lv, y, x, 360.0, 'zonal')
    assert [len(p) for p in polys] == [1, 1, 1] and closed == [[True]] * 3 and wind == [[1]] * 3
    assert [[n for n, _, _ in row] for row in PJ.census(q, lv)] == [[16]] * 3
    for (p,) in polys:                                   # the last vertex is the first, one lap on
        assert p[-1, 0] == p[0, 0] and p[-1, 1] == p[0, 1] + nx and (np.diff(p[:, 1]) >= 0).all()
    (p,) = built(q, lv, y, x, 360.0)[0][0]
    assert p[-1, 0] == p[0, 0] and p[-1, 1] == p[0, 1] + 360.0
    # the other way round: the field negated, or flipped in Y
    for q2, lv2 in ((-q, -lv[::-1]), (q[::-1].copy(), lv)):
        polys, closed, wind = both_ways(q2, lv2, y, x, 360.0, 'zonal reversed')
        assert closed == [[True]] * 3 and wind == [[-1]] * 3
        for (p,) in polys:
            assert p[-1, 1] == p[0, 1] - nx
    # a descending longitude with a negative period
    xd = x[::-1].copy()
    got = built(q, lv, y, xd, -360.0)
    same(got, PJ.polylines(q, lv, y, xd, -360.0), 'descending')
    (p,) = got[0][0]
    assert got[2] == [[1]] * 3 and p[-1, 1] == p[0, 1] - 360.0
    # without the wrap the same levels are open lines
    assert [[(c, w) for _, c, w in row] for row in PJ.census(q, lv, periodic=False)] == [[(False, 0)]] * 3


@pytest.mark.parametrize('centre', [0, 3])
def test_ring_across_the_seam_both_ways_has_laps_but_no_winding(centre):
    """a cone centred on or near column 0: its rings cross the seam twice, once each way.  Centred on column 0 the walk starts on
    the seam and its second pass is the step that closes the ring; centred on column 3 both passes lie inside the walk"""
    import contour_join_ref as JR
    ny, nx = 21, 30
    r, c = np.meshgrid(np.arange(ny) - 10.0, (np.arange(nx) - centre + 15) % nx - 15.0, indexing='ij')
    q = -np.hypot(r, 1.1 * c)
    lv = np.array([-6.3, -4.2])
    y, x = np.arange(ny) * 1.5, 10.0 + np.arange(nx) * 0.5
    polys, closed, wind = both_ways(q, lv, y, x, 15.0, 'cone')
    assert closed == [[True]] * 2 and wind == [[0]] * 2
    for (p,) in polys:
        assert np.array_equal(p[0], p[-1])
        assert (p[:, 1].min() < 0.0 or p[:, 1].max() > nx) and np.abs(np.diff(p[:, 1])).max() <= 1.0      # it runs on past the seam
    for ef, et, pts in PJ.segments(q, lv):
        ((segs, ring),) = JR.join(ef, et)
        laps = PJ.walk_polyline(pts, segs, ring, nx)[2]
        assert ring and laps[0] == 0 and set(laps) in ({0, 1}, {0, -1})
        if centre:
            assert laps[-1] == 0                        # out and back again inside the walk
    # plain tracing leaves open arcs only
    assert all(row and not any(c for _, c, _ in row) for row in PJ.census(q, lv, periodic=False))


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_random_fields_and_nan_cells(seed):
    rng = np.random.default_rng(seed)
    ny, nx = 14, 19
    q = rng.standard_normal((ny, nx)) + 0.6 * np.arange(ny)[:, None]
    lv = np.array([-0.5, 0.0, 2.1, 4.4, 7.7, 30.0])
    y = np.sort(rng.uniform(-80.0, 80.0, ny))
    x = np.sort(rng.uniform(0.0, 350.0, nx))
    both_ways(q, lv, y, x, 360.0, 'random')
    both_ways(q, lv, y[::-1].copy(), x[::-1].copy(), -365.25, 'random, descending')
    qn = q.copy()
    qn[rng.random(q.shape) < 0.06] = np.nan
    qn[3:6, [0, nx - 1]] = np.nan                        # and a hole on the seam itself
    polys, closed, wind = both_ways(qn, lv, y, x, 360.0, 'nan')
    assert any(not c for row in closed for c in row) and polys[-1] == []
    assert all(w == 0 for row, cl in zip(wind, closed) for w, c in zip(row, cl) if not c)
    both_ways(np.full((4, 5), np.nan), lv, y[:4], x[:5], 360.0, 'all NaN')
    both_ways(q[:, :2], lv, y, x[:2], 360.0, 'two columns')


def test_plain_call_of_the_builder_is_the_plain_vertex_rule():
    import contour_join_ref as JR
    rng = np.random.default_rng(5)
    q = rng.standard_normal((11, 13))
    lv = np.array([-0.4, 0.3])
    y, x = np.linspace(0.0, 5.0, 11), np.linspace(-3.0, 3.0, 13)
    cnt, ef, et, pts = JR.stack_records(q[None], lv)
    off = np.concatenate([[0], np.cumsum(cnt.ravel().astype(np.int64))])
    walk, poff, closed, rpo = nat.join_segments(off, ef, et)
    for kw, ref in ((dict(), JR.polylines(q, lv)), (dict(ycoord=y, xcoord=x), JR.polylines(q, lv, y, x))):
        polys, cl, wd = xa.contour_polylines(walk, poff, closed, rpo, pts, **kw)
        same((polys, cl, wd), (ref[0], ref[1], [[0] * len(c) for c in ref[1]]), 'plain')


def test_barotropic_field_periodic_tracing_leaves_one_winding_ring_per_level(baro):
    q = baro[0].astype(np.float64)
    assert q.shape == (256, 512)
    lv = np.linspace(q.min(), q.max(), 9)[1:-1]
    plain = PJ.census(q, lv, periodic=False)
    assert [sum(1 for _, c, _ in row if not c) for row in plain] == [1, 1, 1, 1, 1, 1, 3]
    ring = PJ.census(q, lv)
    assert all(c for row in ring for _, c, _ in row)                                  # no open polyline is left
    assert [[n for n, _, w in row if w != 0] for row in ring] == [[544], [544], [592], [1068], [2284], [652], [2372]]
    assert all(abs(w) <= 1 for row in ring for _, _, w in row)


def _cm(lon, ny=5, coords=True):
    c = {'lat': np.linspace(-40.0, 40.0, ny), 'lon': lon} if coords else {}
    q = xa.DataArray(np.zeros((ny, lon.size)), ('lat', 'lon'), c, 'q')
    return xa.Contour2D(q, np.ones(ny), {'X': 'lon', 'Y': 'lat'}, {'Y': 'lat'})


def test_facade_rejects_bad_periods_before_touching_a_device():
    lon = np.arange(0.0, 360.0, 45.0)                                                # 0 ... 315
    cm, lv = _cm(lon), np.array([0.5])
    for bad, text in ((0.0, 'periodic should be a finite, non-zero period'), (np.nan, 'periodic should be a finite, non-zero period'),
                      (np.inf, 'periodic should be a finite, non-zero period'), (-360.0, 'periodic=-360.0 runs against the X coordinate'),
                      (315.0, 'periodic=315.0 is too short'), (300, 'periodic=300 is too short'),
                      ('ring', 'periodic should be False, True or the period')):
        with pytest.raises(Exception, match='find_contours: ' + text):
            cm.find_contours(lv, periodic=bad)
    with pytest.raises(Exception, match='periodic=True runs against the X coordinate|periodic=360.0 runs against'):
        _cm(lon[::-1].copy()).find_contours(lv, periodic=360.0)
    for index in (False, True):
        with pytest.raises(Exception, match='at least two columns'):
            _cm(lon[:1]).find_contours(lv, periodic=True, index=index)
    with pytest.raises(Exception, match='at least two columns'):
        _cm(lon[:1], coords=False).find_contours(lv, periodic=360.0, index=True)
    with pytest.raises(Exception, match='needs coordinate values'):
        _cm(lon, coords=False).find_contours(lv, periodic=True)


def test_the_period_of_find_contours_is_float64_as_given():
    f = xa.Contour2D._x_period
    lon = np.arange(0.0, 360.0, 45.0)
    assert f(False, lon, False, 'f', plain=True) is None and f(None, lon, False, 'f', plain=True) is None
    assert f(True, lon, False, 'f', plain=True) == 360.0 and f(True, lon[::-1], False, 'f', plain=True) == -360.0
    assert f(400.1, lon, False, 'f', plain=True) == 400.1 and f(400.1, lon, True, 'f', plain=True) == 400.1
    # what K10 and K11 receive is unchanged
    assert f(400.1, lon.astype(np.float32), True, 'f') == float(np.float64(np.deg2rad(np.float32(400.1))))
    with pytest.raises(Exception, match='periodic=True needs latlon=True'):
        f(True, lon, False, 'f')


def test_entry_points_and_signatures_exist():
    lib = nat.load()
    for name in NEW:
        assert name in nat.PROTOTYPES and hasattr(lib, name)
        assert list(nat.PROTOTYPES[name][1]) == list(nat.PROTOTYPES[name.replace('_periodic', '')][1])
    assert inspect.signature(nat.Context.contour_segments).parameters['periodic'].default is False
    p = inspect.signature(xa.Contour2D.find_contours).parameters
    assert list(p)[1:] == ['contours', 'tracer', 'index', 'return_closed', 'periodic', 'return_winding']
    assert p['periodic'].default is False and p['return_winding'].default is False
    p = inspect.signature(xa.find_contour).parameters
    assert list(p) == ['data', 'dims', 'level', 'period', 'periodic'] and p['periodic'].default is False
