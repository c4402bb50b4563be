"""K10 (xc_contour_lengths, Contour2D.cal_contour_lengths) on the GPU against the numpy restatement clength_ref:
segment counts exact, totals within 1e-12, NaN exactly where the restatement's total is 0, sums bit-reproducible."""
import numpy as np
import pytest

import clength_ref as CR
import xcontour_amd as xa
from xcontour_amd import _native as nat

pytestmark = pytest.mark.gpu


def check(lens, cnts, ref_t, ref_n, what=''):
    lens, cnts = np.asarray(lens), np.asarray(cnts)
    assert np.array_equal(cnts.astype(np.int64), ref_n), what
    assert np.array_equal(np.isnan(lens), np.isnan(ref_t)), what
    ok = ~np.isnan(ref_t)
    if ok.any():
        r = np.abs(lens[ok] - ref_t[ok]) / np.abs(ref_t[ok])
        assert r.max() <= 1e-12, '%s: rel %.3g' % (what, r.max())


def ref_stack(q, levels, y, x, latlon):
    out = [CR.contour_lengths(q[s], levels[s] if np.ndim(levels) == 2 else levels, y, x, latlon) for s in range(q.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return np.array_equal(a.view(np.int64), b.view(np.int64))


def latlon_grid(ny, nx):
    lat = np.linspace(-90.0, 90.0, ny)
    lon = np.linspace(0.0, 360.0, nx, endpoint=False)
    return lat, lon


def smooth_field(ny, nx, seed=0, noise=0.0):
    lat, lon = latlon_grid(ny, nx)
    La, Lo = np.meshgrid(np.deg2rad(lat), np.deg2rad(lon), indexing='ij')
    q = np.sin(La) * 2.0 + 0.3 * np.cos(3 * Lo) * np.cos(La) ** 2 + 0.1 * np.sin(5 * Lo + 2 * La)
    if noise:
        q = q + noise * np.random.default_rng(seed).standard_normal(q.shape)
    return q, lat, lon


@pytest.mark.parametrize('dt', [np.float32, np.float64])
def test_closed_forms(ctx, dt):
    lat, lon = np.linspace(-80.0, 80.0, 17), np.arange(0.0, 360.0, 7.5)
    y, x = CR.plane_coords(lat, lon, True)
    q = np.repeat(np.arange(17.0)[:, None] * 3.0, lon.size, axis=1).astype(dt)
    lv = np.array([0.7, 10.1, 25.5, 47.9])
    lens, cnts = ctx.contour_lengths(q[None], lv, y, x, radius=CR.RADIUS)
    check(lens[0], cnts[0], *CR.contour_lengths(q.astype(np.float64), lv, y, x, True))
    assert np.all(cnts[0] == lon.size - 1)
    ny, nx = 13, 21
    yc, xc = np.linspace(0.0, 600.0, ny), np.linspace(0.0, 2000.0, nx)
    col = np.repeat(np.arange(nx, dtype=np.float64)[None, :], ny, axis=0).astype(dt)
    lens, cnts = ctx.contour_lengths(col[None], [3.25, 17.5], yc, xc)
    assert np.array_equal(cnts[0], [ny - 1, ny - 1])
    assert np.allclose(lens[0], 600.0, rtol=1e-12, atol=0)


@pytest.mark.parametrize('kind', ['random', 'nan', 'saddle'])
@pytest.mark.parametrize('dt', [np.float32, np.float64])
def test_matches_restatement(ctx, kind, dt):
    rng = np.random.default_rng(7)
    ny, nx, ns = 97, 301, 3
    if kind == 'saddle':
        q = np.indices((ny, nx)).sum(0) % 2 * 2.0 - 1.0 + 0.3 * rng.standard_normal((ns, ny, nx))    # checkerboard
    else:
        q = rng.standard_normal((ns, ny, nx))
    if kind == 'nan':
        q[rng.random(q.shape) < 0.03] = np.nan
    q = q.astype(dt)
    lat, lon = latlon_grid(ny, nx)
    lv = np.linspace(-2.0, 2.0, 37)
    for latlon in (True, False):
        y, x = CR.plane_coords(lat, lon, latlon) if latlon else (np.linspace(0, 5e5, ny), np.linspace(0, 9e5, nx))
        lens, cnts = ctx.contour_lengths(q, lv, y, x, radius=CR.RADIUS if latlon else 0.0)
        check(lens, cnts, *ref_stack(q.astype(np.float64), lv, y, x, latlon), what='%s latlon=%s' % (kind, latlon))


def test_degenerate_levels(ctx):
    rng = np.random.default_rng(3)
    q = rng.integers(0, 6, size=(2, 40, 70)).astype(np.float64)      # levels exactly on node values
    y, x = np.arange(40.0) * 3.0, np.arange(70.0) * 2.0
    lv = np.array([-1.0, 0.0, 1.0, 2.0, 2.5, 3.0, 4.0, 5.0, 6.0])   # out of range, minimum, on nodes, maximum, above
    lens, cnts = ctx.contour_lengths(q, lv, y, x)
    rt, rn = ref_stack(q, lv, y, x, False)
    check(lens, cnts, rt, rn)
    # below the range, at the maximum and above it nothing is traced; at the minimum only the sides joining two minimum nodes
    assert np.isnan(lens[:, [0, 7, 8]]).all() and (cnts[:, [0, 7, 8]] == 0).all()


def _facade(q, lat, lon, **kw):
    c = {'lat': lat, 'lon': lon}
    tr = xa.DataArray(q, ('lat', 'lon') if q.ndim == 2 else ('time', 'lat', 'lon'),
                      dict(c, **({'time': np.arange(q.shape[0])} if q.ndim == 3 else {})), 'q')
    return xa.Contour2D(tr, np.ones(lat.size), {'X': 'lon', 'Y': 'lat'}, {'Y': 'lat'}, dtype=np.float64, **kw), tr


def test_unsorted_levels_come_back_in_caller_order(ctx):
    q, lat, lon = smooth_field(91, 180, noise=0.05)
    cm, _ = _facade(q, lat, lon)
    lv = np.array([0.5, -1.0, np.nan, 1.5, 0.0, 9.0])
    got = cm.cal_contour_lengths(lv, latlon=True).values
    y, x = CR.plane_coords(lat, lon, True)
    rt, _ = CR.contour_lengths(q, lv, y, x, True)
    assert np.array_equal(np.isnan(got), np.isnan(rt))
    ok = ~np.isnan(rt)
    assert np.max(np.abs(got[ok] - rt[ok]) / rt[ok]) <= 1e-12


def test_barotropic_facade_matches_restatement(baro):
    q, lat, lon = baro
    c = {'latitude': lat, 'longitude': lon}
    tr = xa.DataArray(q, ('latitude', 'longitude'), c, 'absolute_vorticity')
    cm = xa.Contour2D(tr, np.ones(lat.size), {'X': 'longitude', 'Y': 'latitude'}, {'Y': 'latitude'}, dtype=np.float64)
    ctr = cm.cal_contours(121)
    got = cm.cal_contour_lengths(121, latlon=True)
    assert got.dims == ('contour',) and got.values.shape == (121,)
    y, x = CR.plane_coords(lat, lon, True)
    rt, _ = CR.contour_lengths(q.astype(np.float64), ctr.values.astype(np.float64), y, x, True)
    ok = ~np.isnan(rt)
    assert np.array_equal(np.isnan(got.values), ~ok)
    assert np.max(np.abs(got.values[ok] - rt[ok]) / rt[ok]) <= 1e-12


@pytest.mark.parametrize('noise', [0.0, 0.2])
def test_full_slab(ctx, noise):
    q, lat, lon = smooth_field(1801, 3600, noise=noise)
    lv = np.linspace(q.min(), q.max(), 43)[1:-1]
    y, x = CR.plane_coords(lat, lon, True)
    lens, cnts = ctx.contour_lengths(q[None], lv, y, x, radius=CR.RADIUS)
    check(lens[0], cnts[0], *CR.contour_lengths(q, lv, y, x, True), what='noise %g' % noise)


def test_many_levels_past_the_lds_split(ctx):
    rng = np.random.default_rng(11)
    q = rng.standard_normal((2, 120, 257))
    lv = np.sort(rng.uniform(-3.0, 3.0, 3000))
    y, x = np.linspace(0.0, 1e4, 120), np.linspace(0.0, 3e4, 257)
    lens, cnts = ctx.contour_lengths(q, lv, y, x)
    check(lens, cnts, *ref_stack(q, lv, y, x, False))


def test_stack_bits_equal_loop_and_repeat_and_resident(ctx):
    q, lat, lon = smooth_field(181, 360, noise=0.1)
    stack = np.stack([q, q[::-1], 0.5 * q + 0.1, q ** 2])
    y, x = CR.plane_coords(lat, lon, True)
    rng = np.random.default_rng(5)
    ctr = np.sort(rng.uniform(-2.0, 2.0, (4, 57)), axis=1)
    a, na = ctx.contour_lengths(stack, ctr, y, x, radius=CR.RADIUS)
    b, nb = ctx.contour_lengths(stack, ctr, y, x, radius=CR.RADIUS)
    assert bits_equal(a, b) and np.array_equal(na, nb)
    for s in range(4):
        l1, n1 = ctx.contour_lengths(stack[s:s + 1], ctr[s], y, x, radius=CR.RADIUS)
        assert bits_equal(l1[0], a[s]) and np.array_equal(n1[0], na[s])
    check(a, na, *ref_stack(stack, ctr, y, x, True))
    # through the facade: per-slab labelled levels, a resident object (device mirror, _dev entry point) and a plain one
    cm_r, tr = _facade(stack, lat, lon, resident=True)
    cm_h, _ = _facade(stack, lat, lon)
    lab = xa.DataArray(ctr, ('time', 'contour'), {'time': np.arange(4), 'contour': np.arange(57)}, 'ctr')
    r1 = cm_r.cal_contour_lengths(lab, latlon=True).values
    r2 = cm_r.cal_contour_lengths(lab, latlon=True).values
    h = cm_h.cal_contour_lengths(lab, latlon=True).values
    assert bits_equal(r1, r2) and bits_equal(r1, h) and bits_equal(h, a)
    cm_r.close()


def test_bad_input_rejected(ctx):
    q = np.zeros((1, 5, 6))
    y, x = np.arange(5.0), np.arange(6.0)
    for bad in ([0.5, np.nan], [1.0, 0.5]):
        with pytest.raises(nat.XContourHipError) as e:
            ctx.contour_lengths(q, bad, y, x)
        assert e.value.code == nat.XC_EEDGES
    with pytest.raises(nat.XContourHipError) as e:
        ctx.contour_lengths(q, [0.5], np.arange(4.0), x)
    assert e.value.code == nat.XC_EBADARG
    with pytest.raises(nat.XContourHipError) as e:
        ctx.contour_lengths(q, [0.5], y, np.full(6, np.inf))
    assert e.value.code == nat.XC_EBADARG
