"""Contour2D.cal_distance_to_contours / Context.contour_distance (K27) on planes, against cdist_ref on the records of the restated
marching squares (contour_join_ref): on the plane dist BIT FOR BIT, edge, piece and the sign equal; on the sphere
|dist - ref| <= R (1e-13 + 1e-13 ref / R) -- device and numpy sin / cos differ by a few ulp of 1, the distance is 1-Lipschitz in
each end point's displacement, every other step is rounded arithmetic of relative error near 1e-15, and a wrong segment or branch
errs by a grid spacing (1e-3 rad or more) -- with `edge` checked by consistency: the restatement's distance from the node to the
returned segment is the returned dist within the same bound."""
import numpy as np
import pytest

import cdist_cases as CC
import cdist_ref as DR
import clength_ref as CR
import contour_join_periodic_ref as JP
import contour_join_ref as JR
import xcontour_amd as xa
from xcontour_amd.utils import Rearth

pytestmark = pytest.mark.gpu


def facade(q, y, x, lead=()):
    dims = tuple('d%d' % i for i in range(len(lead))) + ('latitude', 'longitude')
    c = {'latitude': y, 'longitude': x}
    c.update({'d%d' % i: np.arange(n) for i, n in enumerate(lead)})
    return xa.Contour2D(xa.DataArray(q, dims, c, 'q'), np.ones(len(y)), {'X': 'longitude', 'Y': 'latitude'}, {'Y': 'latitude'}, dtype=np.float64)


def levels_of(cm, lv):
    return xa.DataArray(np.asarray(lv, dtype=np.float64), ('contour',), {'contour': np.arange(len(lv))}, 'q')


def period_of(periodic, latlon):
    if periodic is None or periodic is False:
        return None
    P = 360.0 if periodic is True else float(periodic)
    return float(np.float64(np.deg2rad(np.float32(P)))) if latlon else P


def restated(q2d, lv, y, x, latlon, periodic, select, nodes=None, **kw):
    """the reference of one plane, the levels in ascending order"""
    fy, fx = CR.plane_coords(y, x, latlon)
    period = period_of(periodic, latlon)
    rec = (JP if period is not None else JR).stack_records(np.asarray(q2d, dtype=np.float64)[None], np.asarray(lv, dtype=np.float64))
    ny, nx = q2d.shape
    return rec, DR.distance(*rec, ny, nx, period is not None, select, fy, fx, period or 0.0, Rearth if latlon else 0.0, nodes=nodes, **kw)


def variants(cm, call):
    """the call as it stands, unpruned, and with one range per group: the same bits"""
    a = call()
    try:
        cm.ctx.set_cdist_prune(False)
        b = call()
        cm.ctx.set_cdist_prune(True)
        cm.ctx.set_cpiece_workspace(1)
        c = call()
    finally:
        cm.ctx.set_cdist_prune(True)
        cm.ctx.set_cpiece_workspace(1 << 30)
    for o, what in ((b, 'unpruned'), (c, 'one range per group')):
        for k in ('distance', 'edge', 'piece'):
            va, vo = np.asarray(a[k].values), np.asarray(o[k].values)
            assert np.array_equal(va.view(np.int64), vo.view(np.int64)), '%s: %s differs' % (what, k)
    return a


@pytest.mark.parametrize('shape,periodic,select', [((37, 45), False, 'all'), ((70, 530), 700.0, 'all'), ((70, 530), 700.0, 'main')],
                         ids=['37x45', '70x530 ring', '70x530 ring main'])
def test_cartesian_planes_bit_for_bit(shape, periodic, select):
    ny, nx = shape
    ring = periodic is not False
    q = CC.smooth(ny, nx, 21 + nx, periodic=ring)
    if ring:
        q = q + 1.5 * (np.arange(ny)[:, None] / (ny - 1) - 0.5)               # a gradient across: circumpolar rings exist
    y, x = np.linspace(-30.0, 40.0, ny), np.linspace(0.0, 690.0, nx) + 3.0
    lv = [-0.2, 0.05, 0.35]
    cm = facade(q, y, x)
    got = variants(cm, lambda: cm.cal_distance_to_contours(levels_of(cm, lv), periodic=periodic, select=select, return_nearest=True))
    rec, ref = restated(q, lv, y, x, False, periodic, xa.Context.OVERTURN_SELECT[select])
    d = got['distance'].values
    assert d.shape == (3, ny, nx)
    assert DR.same_bits(np.where(np.isnan(d), np.inf, d), ref['dist']), int((np.where(np.isnan(d), np.inf, d) != ref['dist']).sum())
    assert np.array_equal(got['edge'].values, ref['edge'])
    # piece: the row of the level's cal_contour_pieces table
    tabs = cm.cal_contour_pieces(levels_of(cm, lv), periodic=periodic)
    for k in range(3):
        fe = np.asarray(tabs[k]['first_edge'])
        has = ref['piece'][k] >= 0
        assert np.array_equal(fe[got['piece'].values[k][has]], ref['piece'][k][has]) and (got['piece'].values[k][~has] == -1).all()
    if select == 'main':
        assert np.isfinite(ref['dist']).any()


def test_golden_field_on_the_sphere(baro):
    q, lat, lon = baro
    q = np.asarray(q, dtype=np.float64)
    q2 = q if q.ndim == 2 else q.reshape((-1,) + q.shape[-2:])[0]
    ny, nx = q2.shape
    lv = [float(np.nanmedian(q2))]
    cm = facade(q2, lat, lon)
    got = variants(cm, lambda: cm.cal_distance_to_contours(levels_of(cm, lv), latlon=True, periodic=True, return_nearest=True))
    nodes = (np.arange(0, ny, 4), np.arange(0, nx, 4))
    rec, ref = restated(q2, lv, lat, lon, True, True, 0, nodes=nodes)
    d = got['distance'].values[0][np.ix_(*nodes)]
    tol = Rearth * (1e-13 + 1e-13 * ref['dist'][0] / Rearth)
    err = np.abs(d - ref['dist'][0])
    print('sphere: max |dist - ref| = %.3e m, bound there %.3e m' % (float(err.max()), float(tol.ravel()[err.argmax()])))
    assert (err <= tol).all()
    # the returned segment is (one of) the nearest: the restatement's distance from every node to it, alone
    e = got['edge'].values[0][np.ix_(*nodes)]
    ef = rec[1]
    at = np.searchsorted(ef, e.ravel())
    assert np.array_equal(ef[at], e.ravel())
    fy, fx = CR.plane_coords(lat, lon, True)
    Y1, X1, Y2, X2 = DR.end_points(rec[3], ny, nx, fy, fx, True, DR.RING)
    PY, PX = [v.ravel() for v in np.meshgrid(fy[nodes[0]], fx[nodes[1]], indexing='ij')]
    c2 = DR.c2_sphere(DR.unit(PY, PX)[:, None, :], DR.unit(Y1[at], X1[at])[:, None, :], DR.unit(Y2[at], X2[at])[:, None, :])[:, 0]
    assert (np.abs(DR.finish(c2, Rearth) - d.ravel()) <= tol.ravel()).all()


def test_small_sphere_plane_every_node():
    ny, nx = 37, 45
    q = CC.smooth(ny, nx, 5, periodic=True) + 1.5 * (np.arange(ny)[:, None] / (ny - 1) - 0.5)
    lat, lon = np.linspace(-85.0, 88.0, ny), np.arange(nx) * (360.0 / nx)
    lv = [-0.3, 0.0, 0.3]
    cm = facade(q, lat, lon)
    for select in ('all', 'main'):
        got = variants(cm, lambda: cm.cal_distance_to_contours(levels_of(cm, lv), latlon=True, periodic=True, select=select, return_nearest=True))
        _, ref = restated(q, lv, lat, lon, True, True, xa.Context.OVERTURN_SELECT[select])
        d = got['distance'].values
        assert np.array_equal(np.isnan(d), np.isinf(ref['dist']))
        ok = np.isfinite(ref['dist'])
        assert (np.abs(d[ok] - ref['dist'][ok]) <= Rearth * (1e-13 + 1e-13 * ref['dist'][ok] / Rearth)).all(), select


def test_level_order_nan_level_stack_float32_and_cap():
    ny, nx = 37, 45
    q = np.stack([CC.smooth(ny, nx, 31), CC.smooth(ny, nx, 32)]).astype(np.float32)
    y, x = np.linspace(0.0, 36.0, ny), np.linspace(5.0, 60.0, nx)
    lv = np.array([[0.3, np.nan, -0.2], [0.1, -0.4, 0.2]])
    cm = facade(q, y, x, lead=(2,))
    ctr = xa.DataArray(lv, ('d0', 'contour'), {'d0': np.arange(2), 'contour': np.arange(3)}, 'q')
    got = cm.cal_distance_to_contours(ctr).values
    assert got.shape == (2, 3, ny, nx) and np.isnan(got[0, 1]).all()
    for s in range(2):
        for k in range(3):
            if np.isnan(lv[s, k]):
                continue
            _, ref = restated(q[s].astype(np.float64), [lv[s, k]], y, x, False, False, 0)
            assert DR.same_bits(np.where(np.isnan(got[s, k]), np.inf, got[s, k]), ref['dist'][0]), (s, k)
    cap = float(np.nanmedian(got[1, 0]))
    capped = cm.cal_distance_to_contours(ctr, max_distance=cap).values
    assert np.array_equal(np.isnan(capped[1, 0]), got[1, 0] > cap) and np.isnan(capped[1, 0]).any()
    keep = ~np.isnan(capped)
    assert np.array_equal(capped[keep], got[keep])
    one = xa.distance_to_contour(xa.DataArray(q[1], ('latitude', 'longitude'), {'latitude': y, 'longitude': x}, 'q'), ['latitude', 'longitude'], 0.1)
    assert DR.same_bits(np.asarray(one.values), got[1, 0])


def test_signed_is_negative_exactly_inside_the_mask():
    ny, nx = 37, 40
    q = CC.ring_field(ny, nx)
    y, x = np.linspace(10.0, 82.0, ny), np.arange(nx) * 9.0
    cm = facade(q, y, x)
    lv = levels_of(cm, [0.0, 2.0])
    for select, side in (('main', 'upper'), ('all', 'lower')):
        plain = cm.cal_distance_to_contours(lv, periodic=360.0, select=select).values
        signed = cm.cal_distance_to_contours(lv, periodic=360.0, select=select, side=side, signed=True).values
        mask = cm.cal_integral_inside_contours(lv, periodic=360.0, select=select, side=side, return_mask=True)['mask'].values
        assert np.array_equal(np.abs(signed), plain) and mask.any() and not mask.all()
        assert np.array_equal(np.signbit(signed) & (plain > 0), mask & (plain > 0))
