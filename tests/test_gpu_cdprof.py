"""Contour2D.cal_contour_distance_profile / Context.contour_distance_profile (K28): composites by distance, against cdprof_ref.  On
the plane every number BIT FOR BIT against the restatement (cdist_ref's distances, np.searchsorted's bins, math.fsum's sums); on the
sphere, where the device's asin need not be numpy's, against K27's own downloaded planes binned on the host -- equal exactly when
K28 runs K27's search.  dA varies along Y, one field has mixed signs and six decades of range: a sum that depended on the order of
its terms would differ."""
import functools
import math

import numpy as np
import pytest

import cdist_cases as CC
import cdprof_ref as PR
import clength_ref as CR
import contour_join_periodic_ref as JP
import contour_join_ref as JR
import xcontour_amd as xa

pytestmark = pytest.mark.gpu

VARS = ('nodes', 'area', 'f1', 'f2')


def weights(ny):
    return 1.0 + 0.37 * np.sin(1.0 + np.arange(ny, dtype=np.float64))


def fields_of(ny, nx, seed):
    rng = np.random.default_rng(seed)
    f1 = rng.normal(size=(ny, nx)) * 10.0 ** rng.uniform(0.0, 6.0, size=(ny, nx))      # mixed signs, six decades
    return f1, CC.smooth(ny, nx, seed + 1)


def facade(q, y, x, lead=()):
    dims = tuple('d%d' % i for i in range(len(lead))) + ('latitude', 'longitude')
    c = {'latitude': y, 'longitude': x}
    c.update({'d%d' % i: np.arange(n) for i, n in enumerate(lead)})
    return xa.Contour2D(xa.DataArray(q, dims, c, 'q'), weights(len(y)), {'X': 'longitude', 'Y': 'latitude'}, {'Y': 'latitude'}, dtype=np.float64)


def levels_of(lv):
    return xa.DataArray(np.asarray(lv, dtype=np.float64), ('contour',), {'contour': np.arange(len(lv))}, 'q')


def plane(a, y, x):
    return xa.DataArray(a, ('latitude', 'longitude'), {'latitude': y, 'longitude': x}, 'f')


def w_plane(ny, nx):
    return np.ascontiguousarray(np.broadcast_to(weights(ny)[:, None], (ny, nx)))


def bits(ds, names=VARS):
    return [np.ascontiguousarray(np.asarray(ds[k].values)).view(np.int64) for k in names]


def variants(cm, call, names=VARS):
    """the call as it stands, unpruned, with one range per group, and with every tile on the global words: the same bits"""
    a = call()
    prof = cm.ctx.last_cdprofile_profile()
    try:
        cm.ctx.set_cdist_prune(False)
        b = call()
        cm.ctx.set_cdist_prune(True)
        cm.ctx.set_cpiece_workspace(1)
        c = call()
        cm.ctx.set_cpiece_workspace(1 << 30)
        cm.ctx.set_cdprofile_global(True)
        d = call()
        forced = cm.ctx.last_cdprofile_profile()
    finally:
        cm.ctx.set_cdist_prune(True)
        cm.ctx.set_cpiece_workspace(1 << 30)
        cm.ctx.set_cdprofile_global(False)
    for o, what in ((b, 'unpruned'), (c, 'one range per group'), (d, 'global path')):
        for k, va, vo in zip(names, bits(a, names), bits(o, names)):
            assert np.array_equal(va, vo), '%s: %s differs' % (what, k)
    assert forced['tiles_window'] == 0 and forced['tiles_global'] == prof['tiles_window'] + prof['tiles_global'] > 0
    return a, prof


def check(got, ref, names=('f1', 'f2')):
    assert np.array_equal(got['nodes'].values, ref['nodes']) and got['nodes'].values.dtype == np.int64
    assert PR.same_bits(got['area'].values, ref['area']), 'area'
    for m, k in enumerate(names):
        assert PR.same_bits(got[k].values, ref['sums'][m]), k
        with np.errstate(all='ignore'):
            mean = np.where(ref['area'] == 0.0, np.nan, ref['sums'][m] / ref['area'])
        assert PR.same_bits(got[k + '_mean'].values, mean), k + '_mean'


# ------------------------------------------------------------------ 1. the hand case: q[y, x] = y, level 2.5
def test_hand_case_unsigned_and_signed():
    ny, nx = 8, 6
    y, x = np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64)
    q = np.repeat(y[:, None], nx, axis=1)
    cm = facade(q, y, x)
    w = w_plane(ny, nx)
    got = cm.cal_contour_distance_profile(levels_of([2.5]), [0.5, 1.5, 2.5])
    assert got['nodes'].dims == ('contour', 'distance_bin') and got['nodes'].values.tolist() == [[12, 24]]
    assert got['area'].values.tolist() == [[math.fsum(w[2:4].ravel()), math.fsum(w[[0, 1, 4, 5]].ravel())]]
    assert got['nodes'].coords['distance_bin'].tolist() == [1.0, 2.0]
    assert got['nodes'].coords['bin_lo'].tolist() == [0.5, 1.5] and got['nodes'].coords['bin_hi'].tolist() == [1.5, 2.5]
    sg = cm.cal_contour_distance_profile(levels_of([2.5]), [-2.5, -0.5, 0.5, 2.5], signed=True)
    assert sg['nodes'].values.tolist() == [[12, 6, 18]]
    assert sg['area'].values.tolist() == [[math.fsum(w[4:6].ravel()), math.fsum(w[3].ravel()), math.fsum(w[0:3].ravel())]]
    lo = cm.cal_contour_distance_profile(levels_of([2.5]), [-2.5, -0.5, 0.5, 2.5], signed=True, side='lower')
    assert lo['nodes'].values.tolist() == [[12, 6, 18]]          # (the counts are symmetric: the areas tell the side)
    assert lo['area'].values.tolist() == [[math.fsum(w[0:2].ravel()), math.fsum(w[2].ravel()), math.fsum(w[3:6].ravel())]]
    one = xa.distance_profile(plane(q, y, x), ['latitude', 'longitude'], 2.5, [0.5, 1.5, 2.5], fields={'f': plane(q, y, x)})
    assert one['nodes'].values.tolist() == [12, 24] and one['area'].values.tolist() == [12.0, 24.0]
    assert one['f'].values.tolist() == [30.0, 6.0 * (0 + 1 + 4 + 5)] and one['f_mean'].values.tolist() == [2.5, 2.5]


# ------------------------------------------------------------------ 2. Cartesian planes, bit for bit
@functools.lru_cache(maxsize=None)
def cartesian(shape, periodic, select):
    ny, nx = shape
    ring = periodic is not False
    q = CC.smooth(ny, nx, 21 + nx, periodic=ring)
    if ring:
        q = q + 1.5 * (np.arange(ny)[:, None] / (ny - 1) - 0.5)
    y, x = np.linspace(-30.0, 40.0, ny), np.linspace(0.0, 690.0, nx) + 3.0
    lv = [-0.2, 0.05, 0.35]
    rec = (JP if ring else JR).stack_records(q[None], np.asarray(lv))
    fy, fx = CR.plane_coords(y, x, False)
    sel = xa.Context.OVERTURN_SELECT[select]
    d = PR.distances(rec, ny, nx, ring, sel, fy, fx, float(periodic) if ring else 0.0)
    return q, y, x, lv, d


@pytest.mark.parametrize('shape,periodic,select', [((37, 45), False, 'all'), ((70, 530), 700.0, 'all'), ((70, 530), 700.0, 'main')],
                         ids=['37x45', '70x530 ring', '70x530 ring main'])
def test_cartesian_bit_for_bit_on_every_path(shape, periodic, select):
    ny, nx = shape
    q, y, x, lv, d = cartesian(shape, periodic, select)
    fin = np.sort(d[np.isfinite(d)])
    assert fin.size
    diag = float(np.hypot(y[-1] - y[0], x[-1] - x[0]))
    on = fin[[fin.size // 7, fin.size // 3, (2 * fin.size) // 3]]              # three edges ON distances of this very case
    edges = np.unique(np.r_[np.linspace(0.0, diag, 9), on])
    assert edges.size == 12 and all((d == v).any() for v in on)
    f1, f2 = fields_of(ny, nx, 5)
    cm = facade(q, y, x)
    call = lambda: cm.cal_contour_distance_profile(levels_of(lv), edges, fields={'f1': plane(f1, y, x), 'f2': plane(f2, y, x)},
                                                   periodic=periodic, select=select)
    got, prof = variants(cm, call)
    ref = PR.profile(d, edges, 3, w_plane(ny, nx), [f1, f2])
    assert ref['nodes'].sum() > 0 and prof['tiles_window'] > 0
    check(got, ref)


# ------------------------------------------------------------------ 3. a tile spans more bins than the LDS window holds
def test_wide_span_takes_the_global_path_unasked():
    q, y, x, lv, d = cartesian((37, 45), False, 'all')
    diag = float(np.hypot(y[-1] - y[0], x[-1] - x[0]))
    edges = np.linspace(0.0, diag, 600)
    f1, f2 = fields_of(37, 45, 6)
    cm = facade(q, y, x)
    got = cm.cal_contour_distance_profile(levels_of(lv), edges, fields={'f1': plane(f1, y, x), 'f2': plane(f2, y, x)})
    prof = cm.ctx.last_cdprofile_profile()
    assert prof['tiles_global'] > 0
    check(got, PR.profile(d, edges, 3, w_plane(37, 45), [f1, f2]))


# ------------------------------------------------------------------ 4. the sphere, against K27's own planes
def k27_reference(cm, lv, edges, ncont, w, fields, **kw):
    d = np.asarray(cm.cal_distance_to_contours(lv, **kw).values, dtype=np.float64)
    d = np.where(np.isnan(d), np.inf, d)
    return PR.profile(d.reshape((-1,) + d.shape[-2:]), edges, ncont, w, fields), d


def test_sphere_signed_main_ring_against_k27s_planes():
    ny, nx = 37, 45
    q = CC.smooth(ny, nx, 5, periodic=True) + 1.5 * (np.arange(ny)[:, None] / (ny - 1) - 0.5)
    lat, lon = np.linspace(-85.0, 88.0, ny), np.arange(nx) * (360.0 / nx)
    lv = levels_of([-0.3, 0.0, 0.3])
    edges = np.array([-8e6, -4e6, -2e6, -5e5, 0.0, 5e5, 2e6, 4e6, 8e6])
    f1, f2 = fields_of(ny, nx, 7)
    cm = facade(q, lat, lon)
    kw = dict(latlon=True, periodic=True, select='main', signed=True)
    got, _ = variants(cm, lambda: cm.cal_contour_distance_profile(lv, edges, fields={'f1': plane(f1, lat, lon), 'f2': plane(f2, lat, lon)}, **kw))
    ref, d = k27_reference(cm, lv, edges, 3, w_plane(ny, nx), [f1, f2], **kw)
    assert (ref['nodes'] > 0).sum() >= 12 and (d < 0).any() and (d > 0).any()
    check(got, ref)


# ------------------------------------------------------------------ 5. the edges of the contract
def test_nan_level_no_contour_cap_stack_order_float32_nan_and_inf():
    ny, nx = 37, 45
    q = np.stack([CC.smooth(ny, nx, 31), CC.smooth(ny, nx, 32)])
    y, x = np.linspace(0.0, 36.0, ny), np.linspace(5.0, 60.0, nx)
    lv = np.array([[0.3, np.nan, -0.2, 99.0], [0.1, -0.4, 0.2, 0.0]])         # out of order; a NaN level; one no contour follows
    edges = np.linspace(0.0, 30.0, 7)
    rng = np.random.default_rng(3)
    f32 = rng.normal(size=(2, ny, nx)).astype(np.float32)
    fnan = rng.normal(size=(ny, nx)); fnan[11, 13] = np.nan
    finf = rng.normal(size=(ny, nx)); finf[20, 7] = np.inf
    cm = facade(q, y, x, lead=(2,))
    ctr = xa.DataArray(lv, ('d0', 'contour'), {'d0': np.arange(2), 'contour': np.arange(4)}, 'q')
    stack = xa.DataArray(f32, ('d0', 'latitude', 'longitude'), {'d0': np.arange(2), 'latitude': y, 'longitude': x}, 'f32')
    flds = {'f32': stack, 'fnan': plane(fnan, y, x), 'finf': plane(finf, y, x)}
    got = cm.cal_contour_distance_profile(ctr, edges, fields=flds)
    assert got['nodes'].values.shape == (2, 4, 6)
    w = w_plane(ny, nx)
    dist = {}
    for s in range(2):
        for k in range(4):
            rec = JR.stack_records(q[s][None], np.array([lv[s, k]])) if not np.isnan(lv[s, k]) else None
            d = PR.distances(rec, ny, nx, False, 0, y, x) if rec is not None else np.full((1, ny, nx), np.inf)
            dist[s, k] = d
            ref = PR.profile(d, edges, 1, w, [f32[s], fnan, finf])
            assert np.array_equal(got['nodes'].values[s, k], ref['nodes'][0]), (s, k)
            assert PR.same_bits(got['area'].values[s, k], ref['area'][0]), (s, k)
            for m, name in enumerate(flds):
                assert PR.same_bits(got[name].values[s, k], ref['sums'][m, 0]), (s, k, name)
    for k in (1, 3):                                                          # the NaN level, the level no contour follows
        assert not got['nodes'].values[0, k].any() and not got['area'].values[0, k].any() and not got['finf'].values[0, k].any()
        assert np.isnan(got['f32_mean'].values[0, k]).all()
    # the NaN node is counted and skipped, the inf node makes its bin of its channel NaN and nothing else
    bn, bi = PR.bins_of(dist[1, 0][0, 11, 13], edges), PR.bins_of(dist[1, 0][0, 20, 7], edges)
    assert bn >= 0 and bi >= 0
    assert np.isfinite(got['fnan'].values[1, 0]).all()
    assert np.flatnonzero(np.isnan(got['finf'].values[1, 0])).tolist() == [int(bi)]
    assert np.isfinite(got['f32'].values).all() and np.isfinite(got['area'].values).all()
    # max_distance inside the edge range: the bins beyond it are empty, the ones below it untouched
    capped = cm.cal_contour_distance_profile(ctr, edges, fields=flds, max_distance=12.0)
    assert not capped['nodes'].values[..., 3:].any() and not capped['area'].values[..., 3:].any()
    assert np.array_equal(capped['nodes'].values[..., :2], got['nodes'].values[..., :2])
    d = np.where(dist[1, 2] > 12.0, np.inf, dist[1, 2])
    assert np.array_equal(capped['nodes'].values[1, 2], PR.profile(d, edges, 1)['nodes'][0])


# ------------------------------------------------------------------ 6. a whole contour set
def test_many_levels_on_the_golden_field(baro):
    q, lat, lon = baro
    q = np.asarray(q, dtype=np.float64)
    q2 = q if q.ndim == 2 else q.reshape((-1,) + q.shape[-2:])[0]
    ny, nx = q2.shape
    lv = np.quantile(q2, np.linspace(0.02, 0.98, 41))
    edges = np.linspace(0.0, 3.0e6, 16)
    f = np.cos(np.deg2rad(lat))[:, None] * np.sin(3.0 * np.deg2rad(lon))[None, :] * 1e3
    cm = facade(q2, lat, lon)
    got = cm.cal_contour_distance_profile(levels_of(lv), edges, fields={'f1': plane(f, lat, lon)}, latlon=True, periodic=True)
    prof = cm.ctx.last_cdprofile_profile()
    assert got['nodes'].values.shape == (41, 15) and prof['tiles_window'] > 0
    w = w_plane(ny, nx)
    for k in range(41):                                                       # K27 level by level, binned on the host
        ref, _ = k27_reference(cm, levels_of(lv[k:k + 1]), edges, 1, w, [f], latlon=True, periodic=True)
        assert np.array_equal(got['nodes'].values[k], ref['nodes'][0]), k
        assert PR.same_bits(got['area'].values[k], ref['area'][0]) and PR.same_bits(got['f1'].values[k], ref['sums'][0, 0]), k
    assert got['nodes'].values.sum() > ny * nx
