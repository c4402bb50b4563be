"""Contour2D.cal_contour_line_integral / cal_contour_line_mean (K15) on the GPU: the barotropic fixture against the numpy
restatement cline_ref at the bars of test_gpu_cline, the mean of the latitude inside every contour's extent, the order of the
levels, the alignment of the integrand."""
import numpy as np
import pytest

import clength_ref as CR
import cline_ref as LR
import xcontour_amd as xa
from test_gpu_cline import check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def case(baro):
    q, lat, lon = baro
    c = {'latitude': lat, 'longitude': lon}
    tr = xa.DataArray(q, ('latitude', 'longitude'), c, 'absolute_vorticity')
    cm = xa.Contour2D(tr, np.ones(lat.size), {'X': 'longitude', 'Y': 'latitude'}, {'Y': 'latitude'}, dtype=np.float64)
    ctr = cm.cal_contours(41)
    rng = np.random.default_rng(61)
    La, Lo = np.meshgrid(np.deg2rad(lat.astype(np.float64)), np.deg2rad(lon.astype(np.float64)), indexing='ij')
    F = 20.0 * np.cos(La) * np.sin(3 * Lo) + 5.0 + rng.standard_normal(q.shape)      # a wind-like field of both signs
    return cm, tr, ctr, F, c


def test_barotropic_integral_and_length_match_restatement(case, baro):
    cm, tr, ctr, F, c = case
    q, lat, lon = baro
    assert q.shape == (256, 512)
    Fd = xa.DataArray(F, ('latitude', 'longitude'), c, 'u')
    integ, length = cm.cal_contour_line_integral(ctr, Fd, latlon=True, periodic=True, return_length=True)
    assert integ.dims == ('contour',) and integ.values.shape == (41,) and length.values.shape == (41,)
    y, x = CR.plane_coords(lat, lon, True)
    P = float(np.float64(np.deg2rad(np.float32(360.0))))
    ref = LR.line_integrals_periodic(q.astype(np.float64), F, ctr.values.astype(np.float64), y, x, P, True)
    check((integ.values, length.values, ref[2]), ref, 'barotropic')
    assert (~np.isnan(ref[0])).sum() >= 35
    only = cm.cal_contour_line_integral(ctr, Fd, latlon=True, periodic=True)
    assert np.array_equal(only.values, integ.values, equal_nan=True)
    assert np.array_equal(length.values, cm.cal_contour_lengths(ctr, latlon=True, periodic=True).values, equal_nan=True)


def test_mean_latitude_lies_inside_every_contours_extent(case, baro):
    cm, tr, ctr, F, c = case
    q, lat, lon = baro
    latb = xa.DataArray(np.repeat(lat.astype(np.float64)[:, None], lon.size, axis=1), ('latitude', 'longitude'), c, 'lat')
    mean = cm.cal_contour_line_mean(ctr, latb, latlon=True, periodic=True).values
    pieces = cm.cal_contour_pieces(ctr, latlon=True, periodic=True)
    seen = 0
    for k in range(41):
        if pieces[k].size == 0:
            assert np.isnan(mean[k])
            continue
        lo, hi = pieces[k]['y_min'].min(), pieces[k]['y_max'].max()
        tol = 1e-12 * max(abs(lo), abs(hi), 1.0)
        assert lo - tol <= mean[k] <= hi + tol, (k, lo, mean[k], hi)
        seen += 1
    assert seen >= 35


def test_levels_in_descending_order_come_back_in_caller_order(case):
    cm, tr, ctr, F, c = case
    Fd = xa.DataArray(F, ('latitude', 'longitude'), c, 'u')
    up = cm.cal_contour_line_integral(ctr, Fd, latlon=True, periodic=True).values
    lv = ctr.values[::-1].copy()
    down = cm.cal_contour_line_integral(xa.DataArray(lv, ('contour',), {'contour': np.arange(41.0)}, 'ctr'), Fd, latlon=True,
                                        periodic=True).values
    assert np.array_equal(down, up[::-1], equal_nan=True) and (~np.isnan(up)).sum() >= 35
    m_up = cm.cal_contour_line_mean(ctr, Fd, latlon=True, periodic=True).values
    m_down = cm.cal_contour_line_mean(xa.DataArray(lv, ('contour',), {'contour': np.arange(41.0)}, 'ctr'), Fd, latlon=True,
                                      periodic=True).values
    assert np.array_equal(m_down, m_up[::-1], equal_nan=True)


def test_transposed_integrand_gives_the_same_result(case):
    cm, tr, ctr, F, c = case
    Fd = xa.DataArray(F, ('latitude', 'longitude'), c, 'u')
    Ft = xa.DataArray(np.ascontiguousarray(F.T), ('longitude', 'latitude'), c, 'u')
    a = cm.cal_contour_line_integral(ctr, Fd, latlon=True, periodic=True).values
    b = cm.cal_contour_line_integral(ctr, Ft, latlon=True, periodic=True).values
    assert np.array_equal(a, b, equal_nan=True)


def test_wrong_shape_or_dims_raise(case, baro):
    cm, tr, ctr, F, c = case
    q, lat, lon = baro
    short = xa.DataArray(F[:-1], ('latitude', 'longitude'), {'latitude': lat[:-1], 'longitude': lon}, 'u')
    with pytest.raises(Exception):
        cm.cal_contour_line_integral(ctr, short, latlon=True, periodic=True)
    other = xa.DataArray(F, ('y', 'longitude'), {'y': lat, 'longitude': lon}, 'u')
    with pytest.raises(Exception):
        cm.cal_contour_line_mean(ctr, other, latlon=True, periodic=True)
    with pytest.raises(Exception):
        cm.cal_contour_line_integral(ctr, F, latlon=True, periodic=True)       # not labelled
