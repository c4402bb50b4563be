"""Contour2D.map_to_plane / cal_equivalent_coordinate_map (K25) on the GPU, on the barotropic fixture: the planes against the
restatement (cmap_ref.contour_map) evaluated on the facade's OWN contour vectors, bit for bit."""
import numpy as np
import pytest

import cmap_ref as R
import xcontour_oracle as O
import xcontour_amd as xa
from gpu_common import same_bits

pytestmark = pytest.mark.gpu

DIMS = ({'X': 'longitude', 'Y': 'latitude'}, {'Y': 'latitude'})
N = 121


def _labelled(q, lat, lon, lead=None):
    c = {'latitude': lat, 'longitude': lon}
    dims = ('latitude', 'longitude')
    if lead is not None:
        c['time'] = lead
        dims = ('time',) + dims
    return xa.DataArray(q, dims, c, 'absolute_vorticity')


def _object(q, lat, lon, increase=True, lt=True, lead=None, **kw):
    tr = _labelled(q, lat, lon, lead)
    dA = xa.DataArray(O.cell_area(lat, lon), ('latitude', 'longitude'), {'latitude': lat, 'longitude': lon}, 'rA')
    mask = xa.DataArray(np.ones((lat.size, lon.size), dtype=q.dtype), ('latitude', 'longitude'), {'latitude': lat, 'longitude': lon}, 'mask')
    cm = xa.Contour2D(tr, dA, dims=DIMS[0], dimEq=DIMS[1], increase=increase, lt=lt, **kw)
    return cm, cm.cal_area_eqCoord_table_hist(mask)


def _stack(v, n):
    """a contour vector of the facade -> (nslab, N) float64"""
    return np.asarray(v.values, dtype=np.float64).reshape(n, -1)


@pytest.mark.parametrize('increase,lt,flip', [(True, True, False), (True, False, False), (False, True, False), (False, False, False),
                                              (False, True, True)], ids=['inc-lt', 'inc-gt', 'dec-lt', 'dec-gt', 'flipped'])
def test_keff_vectors_back_on_the_plane(baro, increase, lt, flip):
    q, lat, lon = baro
    if flip:                                                         # the tracer now decreases with the row index
        q, lat = np.ascontiguousarray(q[::-1]), np.ascontiguousarray(lat[::-1])
    cm, table = _object(q, lat, lon, increase, lt)
    ds = cm.keff(N, table, lat=lat, lon=lon)
    out = cm.map_to_plane(ds['ctr'], {'latEq': ds['latEq'], 'nkeff': ds['nkeff']})
    assert list(out) == ['latEq', 'nkeff']
    ctr = _stack(ds['ctr'], 1)
    ref = R.contour_map(q[None], ctr, [_stack(ds['latEq'], 1), _stack(ds['nkeff'], 1)])
    for k, r in zip(('latEq', 'nkeff'), ref):
        p = out[k]
        assert p.dims == ('latitude', 'longitude') and p.shape == q.shape and p.dtype == np.float64 and p.name == k
        assert np.array_equal(p.coords['latitude'], lat) and np.array_equal(p.coords['longitude'], lon)
        same_bits(p.values, r[0], k)
    # the default float32 levels do not reach the extreme cell: the clamp runs on real data
    q64 = q.astype(np.float64)
    clamped = (q64 > ctr.max()) | (q64 < ctr.min())
    assert clamped.any()
    le = _stack(ds['latEq'], 1)[0]
    ends = np.where(q64 > ctr.max(), le[int(np.argmax(ctr[0]))], le[int(np.argmin(ctr[0]))])
    same_bits(out['latEq'].values[clamped], ends[clamped], 'clamped nodes')
    # where the kernel's own latEq is monotonic, the map is a monotonic function of q
    d = np.diff(le)
    assert (d >= 0).all() or (d <= 0).all()
    m = out['latEq'].values.ravel()[np.argsort(q.ravel(), kind='stable')]
    dm = np.diff(m)
    assert (dm >= 0).all() or (dm <= 0).all()


def test_equivalent_coordinate_map_is_its_composition(baro):
    """on an object with deterministic=True: the histogram sums of two calls of the chain are then the same bits (the default sums are
    LDS atomics in arrival order), so the one call and its four-call composition can be compared bit for bit"""
    q, lat, lon = baro
    cm, table = _object(q, lat, lon, deterministic=True)
    m, disp = cm.cal_equivalent_coordinate_map(N, table, displacement=True)
    ctr = cm.cal_contours(N)
    area = cm.cal_integral_within_contours_hist(ctr)
    eq = table.lookup_coordinates(area)
    m2 = cm.map_to_plane(ctr, eq)
    assert m.name == 'latitudeEq' and m.dims == ('latitude', 'longitude') and disp.name == 'latitudeDisp' and disp.dims == m.dims
    same_bits(m.values, m2.values, 'the four calls')
    same_bits(m.values, R.contour_map(q[None], _stack(ctr, 1), [_stack(eq, 1)])[0][0], 'the restatement')
    same_bits(disp.values, lat.astype(np.float64)[:, None] - m.values, 'displacement')
    same_bits(cm.cal_equivalent_coordinate_map(N, table).values, m.values, 'without displacement')
    # levels instead of a count, and the result of cal_contours itself
    same_bits(cm.cal_equivalent_coordinate_map(ctr, table).values, m.values, 'from cal_contours')
    lev = np.linspace(float(q.min()), float(q.max()), 31)
    c31 = cm.cal_contours(lev)
    m31 = cm.map_to_plane(c31, table.lookup_coordinates(cm.cal_integral_within_contours_hist(c31)))
    same_bits(cm.cal_equivalent_coordinate_map(lev, table).values, m31.values, 'from levels')


def test_time_stack_with_per_slab_levels_equals_single_calls(baro):
    q, lat, lon = baro
    q3 = np.stack([q, q * np.float32(1.5) + np.float32(1e-5), np.roll(q, 37, axis=1) * np.float32(0.5)])
    t = np.arange(3.0)
    cm, table = _object(q3, lat, lon, lead=t)
    ctr = cm.cal_contours(41)
    area = cm.cal_integral_within_contours_hist(ctr)
    assert not np.array_equal(ctr.values[0], ctr.values[1])
    both = cm.map_to_plane(ctr, {'area': area, 'ctr': ctr})
    assert both['area'].dims == ('time', 'latitude', 'longitude') and np.array_equal(both['area'].coords['time'], t)
    for k in range(3):
        one = cm.map_to_plane(ctr.isel({'time': k}), area.isel({'time': k}), tracer=cm.tracer.isel({'time': k}))
        assert one.dims == ('latitude', 'longitude')
        same_bits(both['area'].values[k], one.values, 'step %d' % k)
    ref = R.contour_map(q3, _stack(ctr, 3), [_stack(area, 3), _stack(ctr, 3)])
    same_bits(both['area'].values, ref[0], 'area')
    same_bits(both['ctr'].values, ref[1], 'ctr')
    # in batches of one slab: the same planes
    ctx = cm.ctx
    old = ctx.max_batch_bytes
    try:
        ctx.max_batch_bytes = q.size * (4 + 2 * 8) + 8
        again = cm.map_to_plane(ctr, {'area': area, 'ctr': ctr})
    finally:
        ctx.max_batch_bytes = old
    same_bits(again['area'].values, both['area'].values, 'batched')
    same_bits(again['ctr'].values, both['ctr'].values, 'batched')


def test_resident_tracer_override_and_dtype(baro):
    q, lat, lon = baro
    cm, table = _object(q, lat, lon)
    ctr = cm.cal_contours(N)
    eq = table.lookup_coordinates(cm.cal_integral_within_contours_hist(ctr))
    plain = cm.map_to_plane(ctr, eq)
    rs, _ = _object(q, lat, lon, resident=True)
    try:
        same_bits(rs.map_to_plane(ctr, eq).values, plain.values, 'resident')
        same_bits(rs.map_to_plane(ctr, eq).values, plain.values, 'resident, the mirror in place')
        assert rs.ctx.resident_ptr(rs._memo['tracer'][1][0])
    finally:
        rs.close()
    # tracer= overrides the object's tracer; 1-D levels serve it
    other = _labelled(np.ascontiguousarray(q[:, ::-1] * np.float32(0.75)), lat, lon)
    lev = _stack(ctr, 1)[0]
    got = cm.map_to_plane(lev, eq, tracer=other)
    same_bits(got.values, R.contour_map(other.values[None], lev, [_stack(eq, 1)[0]])[0][0], 'tracer=')
    assert not np.array_equal(got.values, plain.values)
    # dtype=float32: the float64 plane rounded once
    p32 = cm.map_to_plane(ctr, eq, dtype=np.float32)
    assert p32.dtype == np.float32
    same_bits(p32.values, plain.values.astype(np.float32), 'float32')
    # bare arrays
    same_bits(xa.map_to_plane(q, lev, _stack(eq, 1)[0]), plain.values, 'xc.map_to_plane')
