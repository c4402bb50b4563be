"""Contour2D.cal_contour_lengths_coarsened / coarsen / xc.coarsen (K26), the facade, on the GPU: against cal_contour_lengths and
against the context call on the restatement's planes (cscale_ref.py), bit for bit."""
import numpy as np
import pytest

import clength_ref as CR
import cscale_ref as R
from gpu_common import same_bits
import xcontour_amd as xa

pytestmark = pytest.mark.gpu

NAN = np.nan
DIMS = dict(dims={'X': 'lon', 'Y': 'lat'}, dimEq={'Y': 'lat'})


def test_barotropic_field_periodic_sphere(baro):
    q, lat, lon = baro
    tr = xa.DataArray(q, ('latitude', 'longitude'), {'latitude': lat, 'longitude': lon}, 'absolute_vorticity')
    cm = xa.Contour2D(tr, np.ones(lat.size), {'X': 'longitude', 'Y': 'latitude'}, {'Y': 'latitude'}, dtype=np.float64)
    lev = np.quantile(q.astype(np.float64), [0.1, 0.3, 0.5, 0.7, 0.9])
    got = cm.cal_contour_lengths_coarsened(lev, [1, 2, 4], latlon=True, periodic=True)
    assert len(got) == 3 and all(g.dims == ('contour',) and g.shape == (5,) for g in got)
    same_bits(got[0].values, cm.cal_contour_lengths(lev, latlon=True, periodic=True).values, 'ratio 1 is cal_contour_lengths')
    y, x = CR.plane_coords(lat, lon, True)
    period = float(np.float64(np.deg2rad(np.float32(360.0))))                   # the facade's cast rule
    for g, r in zip(got[1:], (2, 4)):
        ref, cnt = cm.ctx.contour_lengths(R.coarsen(q[None], r), lev, R.coarsen_coords(y, r), R.coarsen_coords(x, r), radius=xa.Rearth, period=period)
        assert (cnt > 0).all()
        same_bits(g.values, ref[0], 'ratio %d' % r)
    assert not np.array_equal(got[1].values, got[0].values) and not np.array_equal(got[2].values, got[1].values)
    c = cm.coarsen(4)
    assert c.shape == (64, 128) and c.dtype == np.float64 and c.name == 'absolute_vorticity'
    same_bits(c.values, R.coarsen(q, 4), 'Contour2D.coarsen')
    same_bits(c.coords['latitude'], R.coarsen_coords(lat, 4), 'coarse latitudes: the coordinates as given, float64')
    same_bits(xa.coarsen(tr, ('latitude', 'longitude'), 4).values, c.values, 'xc.coarsen')


def _plane_cm(dtype=np.float32, lead=(), resident=False, seed=3):
    """a 24 x 48 plane (with leading dims) on the coordinates 4.0 * arange: every block mean of ratio 2 and 4 is exact in float32"""
    n = int(np.prod(lead, dtype=np.int64))
    q = R.field(n, 24, 48, dtype, seed=seed).reshape(tuple(lead) + (24, 48))
    names = ('time', 'lev')[:len(lead)]
    c = {d: np.arange(float(k)) for d, k in zip(names, lead)}
    c.update(lat=4.0 * np.arange(24), lon=4.0 * np.arange(48))
    tr = xa.DataArray(q, names + ('lat', 'lon'), c, 'q')
    return xa.Contour2D(tr, np.ones(24), dtype=np.float64, resident=resident, **DIMS), q


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_user_identity_on_exact_coordinates(dtype):
    """every element equals cal_contour_lengths(ctr, tracer=cm.coarsen(r)): what a user would expect.  It holds here because the
    block means of 4.0 * arange are exact in float32; it stops holding for coordinates whose block means need more than float32 --
    cal_contour_lengths casts the coarse coordinates to float32 once more, K26 does not (test_cscale_host.py, f32_coords)"""
    cm, q = _plane_cm(dtype)
    lev = R.levels(R.coarsen(q, 4), 6)
    ratios = [1, 2, 4]
    got = cm.cal_contour_lengths_coarsened(lev, ratios)
    for g, r in zip(got, ratios):
        ref = cm.cal_contour_lengths(lev, tracer=cm.coarsen(r))
        assert np.isfinite(ref.values).sum() >= 3
        same_bits(g.values, ref.values, 'ratio %d' % r)
    nan_q = xa.DataArray(R.with_specials(q, 2), ('lat', 'lon'), dict(lat=4.0 * np.arange(24), lon=4.0 * np.arange(48)), 'q')
    for skipna in (False, True):
        g = cm.cal_contour_lengths_coarsened(lev, 2, tracer=nan_q, skipna=skipna)
        same_bits(g.values, cm.cal_contour_lengths(lev, tracer=cm.coarsen(2, tracer=nan_q, skipna=skipna)).values, 'skipna %d' % skipna)
    # a period in the coordinate's units, Cartesian
    g = cm.cal_contour_lengths_coarsened(lev, [2, 4], periodic=192.0)
    for a, r in zip(g, (2, 4)):
        same_bits(a.values, cm.cal_contour_lengths(lev, tracer=cm.coarsen(r), periodic=192.0).values, 'periodic ratio %d' % r)


def test_caller_level_order_and_nan_levels():
    cm, q = _plane_cm(np.float64)
    lev = R.levels(R.coarsen(q, 4), 6)
    mixed = np.array([lev[4], NAN, lev[0], lev[5], lev[0], lev[2]])
    got = cm.cal_contour_lengths_coarsened(mixed, [2, 4])
    srt = cm.cal_contour_lengths_coarsened(lev, [2, 4])
    for a, b in zip(got, srt):
        assert np.isnan(a.values[1])
        same_bits(a.values[[0, 2, 3, 4, 5]], b.values[[4, 0, 5, 0, 2]], 'the caller\'s order')
        assert np.array_equal(a.coords['contour'], np.arange(6.0))


def test_stack_with_leading_dims_resident_and_ratio_forms():
    cm, q = _plane_cm(np.float32, lead=(2, 3))
    lev = R.levels(R.coarsen(q, 4), 5)
    got = cm.cal_contour_lengths_coarsened(lev, [4, 2])
    assert all(g.dims == ('time', 'lev', 'contour') and g.shape == (2, 3, 5) for g in got)
    for g, r in zip(got, (4, 2)):
        for t in range(2):
            for l in range(3):
                one = cm.ctx.contour_lengths(R.coarsen(q[t, l][None], r), lev, R.coarsen_coords(4.0 * np.arange(24), r),
                                             R.coarsen_coords(4.0 * np.arange(48), r))[0][0]
                same_bits(g.values[t, l], one, 'slab (%d, %d) ratio %d' % (t, l, r))
    c = cm.coarsen(2)
    assert c.dims == ('time', 'lev', 'lat', 'lon') and c.shape == (2, 3, 12, 24)
    same_bits(c.values, R.coarsen(q, 2), 'coarsen with leading dims')
    # per-slab levels
    lab = xa.DataArray(lev[None, None, :] * (1.0 + 0.01 * np.arange(6).reshape(2, 3, 1)), ('time', 'lev', 'contour'),
                       {'time': np.arange(2.0), 'lev': np.arange(3.0), 'contour': np.arange(5.0)}, 'ctr')
    per = cm.cal_contour_lengths_coarsened(lab, [2])[0]
    same_bits(per.values[0, 0], got[1].values[0, 0], 'slab 0 has the shared levels')
    assert not np.array_equal(per.values[1, 2], got[1].values[1, 2])
    # a resident object reads its mirror through the _dev entries
    cr, _ = _plane_cm(np.float32, lead=(2, 3), resident=True)
    for a, b in zip(cr.cal_contour_lengths_coarsened(lev, [4, 2]), got):
        same_bits(a.values, b.values, 'resident')
    same_bits(cr.coarsen(2).values, c.values, 'resident coarsen')
    cr.close()
    # a bare int, and ten ratios in two calls
    same_bits(cm.cal_contour_lengths_coarsened(lev, 2).values, got[1].values, 'a bare int')
    ten = cm.cal_contour_lengths_coarsened(lev, [1, 2, 3, 4, 6, 8, 12, 2, 4, 1])
    assert len(ten) == 10
    for k, j in ((7, 1), (8, 3), (9, 0)):
        same_bits(ten[k].values, ten[j].values, 'ratio repeated across the two calls')
    same_bits(ten[1].values, got[1].values, 'ratio 2')
    same_bits(ten[3].values, got[0].values, 'ratio 4')
    assert xa.fractal_dimension(np.stack([t.values for t in ten[:4]]), [1.0, 2.0, 3.0, 4.0]).shape == (2, 3, 5)
