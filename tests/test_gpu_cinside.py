"""Contour2D.cal_integral_inside_contours (K17) on the GPU, through the facade, on the golden barotropic field with periodic=True
at 21 levels.  'all' must reproduce the threshold mask relative to the first row exactly, and its area math.fsum of dA over that
mask bit for bit; 'main' must flip down every column as often as cal_contour_overturning counts crossings there."""
import math

import numpy as np
import pytest

import xcontour_amd as xa
import xcontour_oracle as O
from test_gpu_parity import rel, TIGHT

pytestmark = pytest.mark.gpu

NLEV = 21


@pytest.fixture(scope='module')
def case(baro):
    q, lat, lon = (np.asarray(a) for a in baro)
    q = q.astype(np.float64)
    c = {'latitude': lat, 'longitude': lon}
    dA = O.cell_area(lat, lon)
    cm = xa.Contour2D(xa.DataArray(q, ('latitude', 'longitude'), c, 'q'), xa.DataArray(dA, ('latitude', 'longitude'), c, 'dA'),
                      {'X': 'longitude', 'Y': 'latitude'}, {'Y': 'latitude'}, dtype=np.float64)
    lv = np.linspace(float(q.min()), float(q.max()), NLEV)
    lv[7] = q[40, 100]                                                       # a level ON a node's value
    lv = np.sort(lv)
    ascends = bool(lat[-1] >= lat[0])
    above = q[None] > lv[:, None, None]
    return dict(q=q, lat=lat, lon=lon, dA=np.asarray(dA, dtype=np.float64), cm=cm, lv=lv, ascends=ascends, above=above)


@pytest.mark.parametrize('side', ['upper', 'lower'])
def test_all_is_the_threshold_mask_and_its_area_the_fsum_of_dA(case, side):
    cm, lv, q, dA, above = case['cm'], case['lv'], case['q'], case['dA'], case['above']
    flip = (side == 'upper') != case['ascends']
    ds = cm.cal_integral_inside_contours(lv, periodic=True, select='all', side=side, return_mask=True)
    assert list(ds) == ['area', 'nodes', 'mask']
    mask = ds['mask'].values
    assert mask.dtype == np.bool_ and mask.shape == (NLEV,) + q.shape and ds['mask'].dims == ('contour', 'latitude', 'longitude')
    expect = above ^ above[:, :1] ^ flip
    assert np.array_equal(mask, expect)
    assert np.array_equal(ds['nodes'].values, expect.reshape(NLEV, -1).sum(axis=1)) and ds['nodes'].values.dtype == np.int64
    assert ds['area'].values.tolist() == [math.fsum(dA[m].tolist()) for m in expect]
    # where the first row lies wholly on one side of the level, one of the two sides IS the reference's threshold region: its
    # cal_integral_within_contours (q > c here: lt=False) sums in another order, so the tolerance is the one the facade tests
    # hold that method to (test_gpu_parity.TIGHT)
    strict = cm.cal_integral_within_contours(lv).values
    row0 = above[:, 0]
    want = row0.all(axis=1) if flip else ~row0.any(axis=1)                   # this side is the region q > c at these levels
    assert (~row0.any(axis=1)).sum() + row0.all(axis=1).sum() >= 3
    assert all(np.array_equal(m, a) for m, a in zip(mask[want], above[want]))
    if want.any():
        assert rel(ds['area'].values[want], strict[want]) < TIGHT


def test_main_flips_down_every_column_as_often_as_k16_counts_crossings(case):
    cm, lv = case['cm'], case['lv']
    ds = cm.cal_integral_inside_contours(lv, periodic=True, select='main', return_mask=True)
    mask = ds['mask'].values
    flips = (mask[:, 1:] != mask[:, :-1]).sum(axis=1)
    over = cm.cal_contour_overturning(lv, periodic=True, select='main')
    assert np.array_equal(flips, over['ncross'].values)
    assert (over['ncross'].values >= 3).any() and (over['main_first_edge'].values >= 0).sum() >= 10
    # the main ring alone bounds less (or other) than all pieces together somewhere: the selection matters on this field
    every = cm.cal_integral_inside_contours(lv, periodic=True, select='all', return_mask=True)
    assert (every['mask'].values != mask).any()
    none = over['main_first_edge'].values < 0
    first_side = mask[:, 0, 0]
    assert (mask[none] == first_side[none][:, None, None]).all()             # no main ring: the whole plane on one side


def test_the_two_sides_are_complements_and_a_second_call_gives_the_same_bits(case):
    cm, lv, q = case['cm'], case['lv'], case['q']
    g = xa.DataArray(np.asarray(q * q), ('latitude', 'longitude'), {'latitude': case['lat'], 'longitude': case['lon']}, 'q2')
    up = cm.cal_integral_inside_contours(lv, integrand=g, periodic=True, side='upper', return_mask=True)
    lo = cm.cal_integral_inside_contours(lv, integrand=g, periodic=True, side='lower', return_mask=True)
    assert list(up) == ['area', 'nodes', 'integral', 'mask']
    assert np.array_equal(up['mask'].values, ~lo['mask'].values)
    assert np.array_equal(up['nodes'].values + lo['nodes'].values, np.full(NLEV, q.size))
    dA = case['dA']
    assert up['integral'].values.tolist() == [math.fsum((dA[m] * (q * q)[m]).tolist()) for m in up['mask'].values]
    again = cm.cal_integral_inside_contours(lv, integrand=g, periodic=True, side='upper', return_mask=True)
    for name in ('area', 'nodes', 'integral', 'mask'):
        assert up[name].values.tobytes() == again[name].values.tobytes(), name
    bare = cm.cal_integral_inside_contours(lv, integrand=g, periodic=True, side='upper')
    assert list(bare) == ['area', 'nodes', 'integral'] and bare['area'].values.tobytes() == up['area'].values.tobytes()


def test_caller_order_a_leading_dim_and_the_refusals(case):
    """the layout of cal_contour_overturning: levels where the caller put them, a NaN level with nothing, leading dims in front"""
    rng = np.random.default_rng(44)
    q = rng.standard_normal((3, 9, 12))
    q[:, 4:] += 3.0
    y, x = np.arange(9) * 1.5 - 6.0, np.arange(12) * 30.0
    lv = np.array([2.1, -0.8, 1.5, np.nan, 0.1])
    order = np.argsort(np.where(np.isnan(lv), np.inf, lv), kind='stable')
    for yc in (y, y[::-1].copy()):
        c = {'latitude': yc, 'longitude': x, 'd0': np.arange(3)}
        dA = rng.random((9, 12)) + 0.5
        cm = xa.Contour2D(xa.DataArray(q, ('d0', 'latitude', 'longitude'), c, 'q'), xa.DataArray(dA, ('latitude', 'longitude'), c, 'dA'),
                          {'X': 'longitude', 'Y': 'latitude'}, {'Y': 'latitude'}, dtype=np.float64)
        ds = cm.cal_integral_inside_contours(lv, periodic=True, select='all', return_mask=True)
        assert ds['area'].dims == ('d0', 'contour') and ds['mask'].dims == ('d0', 'contour', 'latitude', 'longitude')
        assert ds['mask'].values.shape == (3, 5, 9, 12) and np.array_equal(ds['mask'].coords['longitude'], x)
        flip = not bool(yc[-1] >= yc[0])
        with np.errstate(invalid='ignore'):
            above = q[:, None] > lv[None, :, None, None]
        assert np.array_equal(ds['mask'].values, above ^ above[:, :, :1] ^ flip)
        assert ds['area'].values.tolist() == [[math.fsum(dA[m].tolist()) for m in row] for row in ds['mask'].values]
        raw = cm.ctx.contour_interior(q, np.where(np.isnan(lv), np.inf, lv)[order], w=dA, periodic=True, select='all', flip=flip)
        assert np.array_equal(ds['nodes'].values[:, order], raw[0]) and raw[2] is None and len(raw) == 3
        assert (ds['nodes'].values[:, 3] == (9 * 12 if flip else 0)).all()
        plain = cm.cal_integral_inside_contours(lv, select='all', return_mask=True)
        assert np.array_equal(plain['mask'].values, ds['mask'].values)          # NaN-free: the seam cell adds no vertical edge
        with pytest.raises(Exception, match='periodic'):
            cm.cal_integral_inside_contours(lv)
        with pytest.raises(Exception, match='select'):
            cm.cal_integral_inside_contours(lv, periodic=True, select='largest')
        with pytest.raises(Exception, match='side'):
            cm.cal_integral_inside_contours(lv, periodic=True, side='north')
