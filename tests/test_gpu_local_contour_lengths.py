"""K11 (xc_local_contour_lengths, Contour2D.cal_local_contour_lengths) on the GPU against the numpy restatement
local_clength_ref: the windows' mean levels bit for bit, segment counts exact, totals within 1e-12 (K10's bound against the same
restatement), NaN exactly where it has NaN, and sums that do not depend on stride, stacking, batching or the resident path."""
import math

import numpy as np
import pytest

import clength_ref as CR
import local_clength_ref as LR
import xcontour_amd as xa
from xcontour_amd import _native as nat

pytestmark = pytest.mark.gpu


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return np.array_equal(a.view(np.int64), b.view(np.int64))


def check(lens, cnts, ref_t, ref_n, what=''):
    lens, cnts = np.asarray(lens), np.asarray(cnts).astype(np.int64)
    assert np.array_equal(cnts, ref_n), what
    assert np.array_equal(np.isnan(lens), np.isnan(ref_t)), what
    ok = ~np.isnan(ref_t)
    if ok.any():
        r = np.abs(lens[ok] - ref_t[ok]) / np.abs(ref_t[ok])
        print('%s: %d windows, %d with a contour, max rel %.3g' % (what, ref_t.size, ok.sum(), r.max()))
        assert r.max() <= 1e-12, '%s: rel %.3g' % (what, r.max())


def check_stack(q, lens, lvls, cnts, y, x, window, stride, latlon, what=''):
    """the restatement on the levels the GPU returned"""
    for s in range(q.shape[0]):
        rt, rn = LR.local_contour_lengths(q[s].astype(np.float64), lvls[s], y, x, window, stride, latlon)
        check(lens[s], cnts[s], rt, rn, '%s slab %d' % (what, s))


def field(kind, shape, seed, dt=np.float64):
    rng = np.random.default_rng(seed)
    ny, nx = shape[-2:]
    if kind == 'saddle':
        q = np.indices((ny, nx)).sum(0) % 2 * 2.0 - 1.0 + 0.3 * rng.standard_normal(shape)    # checkerboard
    elif kind == 'node':
        q = rng.integers(0, 6, size=shape).astype(np.float64)                                  # levels fall on node values
    else:
        q = rng.standard_normal(shape)
    if kind == 'nan':
        q[rng.random(shape) < 0.08] = np.nan
    return q.astype(dt)


def coords(ny, nx, latlon):
    """coordinates whose spacings differ in every cell; latitude descending on the sphere"""
    if latlon:
        return (np.deg2rad(CR.hashed_coords(ny, 1, -80.0, 160.0 / ny, descending=True)),
                np.deg2rad(CR.hashed_coords(nx, 2, 0.0, 300.0 / nx)))
    return CR.hashed_coords(ny, 3, 5.0, 7.0), CR.hashed_coords(nx, 4, -3.0, 2.0)


# ------------------------------------------------------------------ the means
@pytest.mark.parametrize('window,stride', [((7, 9), (3, 4)), ((6, 4), (5, 2)), ((21, 20), (7, 6))])
@pytest.mark.parametrize('kind', ['random', 'nan'])
@pytest.mark.parametrize('dt', [np.float32, np.float64])
def test_mean_levels_bit_for_bit(ctx, dt, kind, window, stride):
    ny, nx, ns = 37, 53, 2
    q = field(kind, (ns, ny, nx), 11, dt)
    y, x = coords(ny, nx, False)
    n_full = window[0] * window[1]
    for mp in (1, n_full - 3, n_full):                       # met everywhere / missed where NaNs or the edges bite / the default
        lens, lvls, cnts = ctx.local_contour_lengths(q, y, x, window, stride, mp)
        for s in range(ns):
            ref = LR.window_levels(q[s].astype(np.float64), window, stride, mp)
            assert bits_equal(lvls[s], ref), (mp, s)
            miss = np.isnan(ref)
            assert np.isnan(lens[s][miss]).all() and (cnts[s][miss] == 0).all()
        if mp == 1:
            assert not np.isnan(lvls).any()
        if mp == n_full:                                     # windows clipped at each of the four edges miss the full count
            assert np.isnan(lvls[:, 0]).all() and np.isnan(lvls[:, :, 0]).all()
            assert np.isnan(lvls[:, -1]).all() and np.isnan(lvls[:, :, -1]).all()
            assert (~np.isnan(lvls)).any() or kind == 'nan'


# ------------------------------------------------------------------ the lengths
@pytest.mark.parametrize('latlon', [False, True])
@pytest.mark.parametrize('kind', ['random', 'saddle', 'node', 'nan'])
def test_lengths_match_restatement_at_the_means(ctx, kind, latlon):
    ny, nx, ns = 41, 67, 2
    q = field(kind, (ns, ny, nx), 5 + len(kind))
    y, x = coords(ny, nx, latlon)
    window, stride = (9, 12), (4, 5)
    lens, lvls, cnts = ctx.local_contour_lengths(q, y, x, window, stride, 1, radius=CR.RADIUS if latlon else 0.0)
    assert cnts.sum() > 0
    check_stack(q, lens, lvls, cnts, y, x, window, stride, latlon, '%s latlon=%s' % (kind, latlon))


@pytest.mark.parametrize('dt', [np.float32, np.float64])
@pytest.mark.parametrize('latlon', [False, True])
def test_given_levels_per_window_and_scalar(ctx, latlon, dt):
    ny, nx, ns = 33, 58, 3
    window, stride = (8, 11), (3, 7)
    y, x = coords(ny, nx, latlon)
    radius = CR.RADIUS if latlon else 0.0
    nwy, nwx = LR.centres(ny, stride[0]).size, LR.centres(nx, stride[1]).size
    rng = np.random.default_rng(2)
    for kind in ('random', 'node'):
        q = field(kind, (ns, ny, nx), 8, dt)
        per = rng.integers(0, 6, size=(ns, nwy, nwx)).astype(np.float64) if kind == 'node' else rng.uniform(-1.5, 1.5, (ns, nwy, nwx))
        per[0, 1, 2] = np.nan                                # a NaN level: NaN length, 0 segments
        for lv in (per, 2.0 if kind == 'node' else 0.25):
            lens, lvls, cnts = ctx.local_contour_lengths(q, y, x, window, stride, 1, levels=lv, radius=radius)
            assert bits_equal(lvls, np.broadcast_to(np.asarray(lv, dtype=np.float64), lvls.shape))
            check_stack(q, lens, lvls, cnts, y, x, window, stride, latlon, '%s given latlon=%s' % (kind, latlon))
        shared = ctx.local_contour_lengths(q, y, x, window, stride, 1, levels=per[1], radius=radius)      # (nwy, nwx): every slab
        assert bits_equal(shared[1], np.broadcast_to(per[1], shared[1].shape))


# ------------------------------------------------------------------ K10 and reproducibility
@pytest.mark.parametrize('latlon', [False, True])
def test_whole_plane_window_is_k10(ctx, latlon):
    ny, nx = 120, 257
    q = field('random', (2, ny, nx), 21)
    y, x = coords(ny, nx, latlon)
    radius = CR.RADIUS if latlon else 0.0
    # one centre, node (0, 0): an even window of 2 n nodes starts at -n and ends at n - 1, the whole plane after clipping
    for lv in (0.3, -1.1):
        lens, lvls, cnts = ctx.local_contour_lengths(q, y, x, (2 * ny, 2 * nx), (ny, nx), 1, levels=lv, radius=radius)
        assert lens.shape == (2, 1, 1)
        k10, n10 = ctx.contour_lengths(q, [lv], y, x, radius=radius)
        assert np.array_equal(cnts[:, 0, 0], n10[:, 0])
        r = np.abs(lens[:, 0, 0] - k10[:, 0]) / k10[:, 0]
        assert r.max() <= 1e-12
        assert bits_equal(lens[:, 0, 0], k10[:, 0])              # K10's fixed-point sums on K10's window constant: the same integers
        for s in range(2):
            rt, rn = CR.contour_lengths(q[s], [lv], y, x, latlon)
            check(lens[s, 0], cnts[s, 0], rt, rn, 'whole plane')


def test_bits_do_not_depend_on_stride_stack_batches_or_residency(ctx):
    ny, nx, ns = 61, 90, 5
    q = field('nan', (ns, ny, nx), 33)
    lat, lon = np.linspace(-75.0, 75.0, ny), np.linspace(0.0, 356.0, nx)
    y, x = CR.plane_coords(lat, lon, True)
    window = (21, 21)
    a = ctx.local_contour_lengths(q, y, x, window, (5, 5), 200, radius=CR.RADIUS)
    b = ctx.local_contour_lengths(q, y, x, window, (10, 10), 200, radius=CR.RADIUS)
    assert np.nansum(a[2]) > 0
    for u, v in zip(a, b):                                   # stride 10's windows are every other one of stride 5's
        assert bits_equal(u[:, ::2, ::2].astype(np.float64), v.astype(np.float64))
    for s in range(ns):                                      # one slab per call
        one = ctx.local_contour_lengths(q[s:s + 1], y, x, window, (5, 5), 200, radius=CR.RADIUS)
        assert all(bits_equal(u[0].astype(np.float64), v[s].astype(np.float64)) for u, v in zip(one, a))
    old = ctx.max_batch_bytes
    per = ny * nx * 8 + 4 * a[0][0].size * 8
    try:
        for nb in (1, 2, 3):                                 # batches of 1, 2 and 3 slabs: split at different points
            ctx.max_batch_bytes = nb * per + 8
            c = ctx.local_contour_lengths(q, y, x, window, (5, 5), 200, radius=CR.RADIUS)
            assert all(bits_equal(u.astype(np.float64), v.astype(np.float64)) for u, v in zip(c, a)), nb
    finally:
        ctx.max_batch_bytes = old
    # the facade: a resident object (device mirror, _dev entry point) against numpy-in
    tr = xa.DataArray(q, ('time', 'lat', 'lon'), {'time': np.arange(ns), 'lat': lat, 'lon': lon}, 'q')
    kw = dict(stride=5, min_periods=200, latlon=True, return_levels=True)
    cm_r = xa.Contour2D(tr, np.ones(ny), {'X': 'lon', 'Y': 'lat'}, {'Y': 'lat'}, dtype=np.float64, resident=True)
    cm_h = xa.Contour2D(tr, np.ones(ny), {'X': 'lon', 'Y': 'lat'}, {'Y': 'lat'}, dtype=np.float64)
    r1, l1 = cm_r.cal_local_contour_lengths(21, **kw)
    r2, l2 = cm_r.cal_local_contour_lengths(21, **kw)
    h, lh = cm_h.cal_local_contour_lengths(21, **kw)
    assert bits_equal(r1.values, r2.values) and bits_equal(r1.values, h.values) and bits_equal(h.values, a[0])
    assert bits_equal(l1.values, lh.values) and bits_equal(lh.values, a[1]) and bits_equal(l1.values, l2.values)
    cm_r.close()


# ------------------------------------------------------------------ sizes
def smooth_field(ny, nx, seed=0, noise=0.0):
    """the PV-like field of K10's full-size test"""
    lat = np.linspace(-90.0, 90.0, ny)
    lon = np.linspace(0.0, 360.0, nx, endpoint=False)
    La, Lo = np.meshgrid(np.deg2rad(lat), np.deg2rad(lon), indexing='ij')
    q = np.sin(La) * 2.0 + 0.3 * np.cos(3 * Lo) * np.cos(La) ** 2 + 0.1 * np.sin(5 * Lo + 2 * La)
    if noise:
        q = q + noise * np.random.default_rng(seed).standard_normal(q.shape)
    return q, lat, lon


def test_full_slab_sample(ctx):
    ny, nx = 1801, 3600
    q, lat, lon = smooth_field(ny, nx, noise=0.2)
    y, x = CR.plane_coords(lat, lon, True)
    window, stride = (101, 101), (10, 10)
    lens, lvls, cnts = ctx.local_contour_lengths(q[None], y, x, window, stride, 1, radius=CR.RADIUS)
    nwy, nwx = 181, 360
    assert lens.shape == (1, nwy, nwx)
    rng = np.random.default_rng(17)
    edge_j, edge_i = [0, 1, 4, 5, nwy - 6, nwy - 5, nwy - 2, nwy - 1], [0, 2, 4, 5, nwx - 6, nwx - 5, nwx - 3, nwx - 1]
    sample = {(a, b) for a in (0, nwy - 1) for b in (0, nwx - 1)}                                  # the four corners
    sample |= {(a, int(b)) for a in edge_j for b in rng.integers(0, nwx, 6)}                       # top and bottom edges
    sample |= {(int(a), b) for b in edge_i for a in rng.integers(0, nwy, 6)}                       # left and right edges
    sample |= {(int(a), int(b)) for a, b in zip(rng.integers(0, nwy, 130), rng.integers(0, nwx, 130))}
    sample = sorted(sample)
    assert len(sample) >= 200
    jj, ii = np.array([s[0] for s in sample]), np.array([s[1] for s in sample])
    (r0, r1), (c0, c1) = LR.bounds(ny, 101, 10), LR.bounds(nx, 101, 10)
    for a, b in sample:
        assert bits_equal(lvls[0, a, b], LR.sequential_mean(q[r0[a]:r1[a] + 1, c0[b]:c1[b] + 1], 1)), (a, b)
    rt, rn = LR.local_contour_lengths(q, lvls[0], y, x, window, stride, True, sample=sample)
    check(lens[0][jj, ii], cnts[0][jj, ii], rt[jj, ii], rn[jj, ii], 'full slab')
    assert (rn[jj, ii] > 0).sum() > 150


def test_plane_smaller_than_window_and_smallest_window(ctx):
    q = field('random', (2, 7, 5), 3)
    y, x = coords(7, 5, False)
    lens, lvls, cnts = ctx.local_contour_lengths(q, y, x, (12, 9), (2, 3), 1)        # every window is clipped, some are the whole plane
    assert lens.shape == (2, 4, 2)
    for s in range(2):
        assert bits_equal(lvls[s], LR.window_levels(q[s], (12, 9), (2, 3), 1))
    check_stack(q, lens, lvls, cnts, y, x, (12, 9), (2, 3), False, 'small plane')
    q = field('saddle', (1, 19, 23), 9)
    y, x = coords(19, 23, True)
    lens, lvls, cnts = ctx.local_contour_lengths(q, y, x, (2, 2), (1, 1), 4, radius=CR.RADIUS)      # one cell per window
    assert bits_equal(lvls[0], LR.window_levels(q[0], (2, 2), (1, 1), 4))
    assert np.isnan(lvls[0, 0]).all() and np.isnan(lvls[0, :, 0]).all() and cnts[0, 1:, 1:].min() >= 1
    check_stack(q, lens, lvls, cnts, y, x, (2, 2), (1, 1), True, '2 x 2')
    for plane in ((1, 1, 6), (1, 6, 1)):                                              # no cells at all
        lens, lvls, cnts = ctx.local_contour_lengths(np.ones(plane), np.arange(plane[1] * 1.0), np.arange(plane[2] * 1.0), (3, 3), (1, 1), 1)
        assert np.isnan(lens).all() and (lvls == 1.0).all() and (cnts == 0).all()


def test_bad_input_rejected(ctx):
    q = np.zeros((1, 5, 6))
    y, x = np.arange(5.0), np.arange(6.0)
    for args in ((y, x, (1, 3), (1, 1), 1), (y, x, (3, 3), (0, 1), 1), (np.arange(4.0), x, (3, 3), (1, 1), 1),
                 (y, np.full(6, np.inf), (3, 3), (1, 1), 1)):
        with pytest.raises(nat.XContourHipError) as e:
            ctx.local_contour_lengths(q, *args)
        assert e.value.code == nat.XC_EBADARG
    with pytest.raises(nat.XContourHipError) as e:
        ctx.local_contour_lengths(q, y, x, (3, 3), (1, 1), 1, levels=np.zeros((2, 2)))
    assert e.value.code == nat.XC_EBADARG


# ------------------------------------------------------------------ the facade
def test_facade_labels_and_latitude_arcs(ctx):
    ny, nx = 46, 80
    lat, lon = np.linspace(-67.5, 67.5, ny), np.arange(nx) * 4.5
    q = field('random', (3, ny, nx), 13, np.float32)
    tr = xa.DataArray(q, ('time', 'lat', 'lon'), {'time': np.arange(3), 'lat': lat, 'lon': lon}, 'q')
    cm = xa.Contour2D(tr, np.ones(ny), {'X': 'lon', 'Y': 'lat'}, {'Y': 'lat'}, dtype=np.float32)
    out, lv = cm.cal_local_contour_lengths({'lat': 9, 'lon': 11}, stride={'lat': 4, 'lon': 5}, min_periods=1, latlon=True,
                                           return_levels=True)
    assert out.dims == ('time', 'lat', 'lon') and lv.dims == out.dims
    assert out.values.shape == (3, 12, 16) and out.values.dtype == np.float32 and lv.values.dtype == np.float64
    assert np.array_equal(out.coords['lat'], lat[::4]) and np.array_equal(out.coords['lon'], lon[::5])
    assert np.array_equal(out.coords['time'], np.arange(3))
    y, x = CR.plane_coords(lat, lon, True)
    for s in range(3):
        assert bits_equal(lv.values[s], LR.window_levels(q[s].astype(np.float64), (9, 11), (4, 5), 1))
        rt, _ = LR.local_contour_lengths(q[s].astype(np.float64), lv.values[s], y, x, (9, 11), (4, 5), True)
        assert np.array_equal(np.isnan(out.values[s]), np.isnan(rt))
        ok = ~np.isnan(rt)                                   # float64 totals within 1e-12 round to float32 values at most one ulp apart
        assert np.max(np.abs(out.values[s][ok].astype(np.float64) - rt[ok]) / rt[ok]) <= 2.0 ** -23
    # the latitude field as the tracer: the window's mean latitude is traced, an arc of that latitude across the window
    latf = xa.DataArray(np.repeat(lat[:, None], nx, axis=1), ('lat', 'lon'), {'lat': lat, 'lon': lon}, 'lat2d')
    cm64 = xa.Contour2D(tr, np.ones(ny), {'X': 'lon', 'Y': 'lat'}, {'Y': 'lat'}, dtype=np.float64)
    arc, lvl = cm64.cal_local_contour_lengths(9, stride=4, min_periods=1, tracer=latf, latlon=True, return_levels=True)
    assert arc.dims == ('lat', 'lon') and arc.values.shape == (12, 20)
    (r0, r1), (c0, c1) = LR.bounds(ny, 9, 4), LR.bounds(nx, 9, 4)
    latv = lat.astype(np.float64)
    for a in range(12):
        for b in range(20):
            if r1[a] - r0[a] != 8 or c1[b] - c0[b] != 8:
                continue                                                          # interior windows
            c = lvl.values[a, b]
            r = int(np.searchsorted(latv, c, 'right')) - 1                       # lat[r] <= c < lat[r + 1]
            f = (c - latv[r]) / (latv[r + 1] - latv[r])
            yy = (y[r + 1] - y[r]) * f + y[r]
            want = math.fsum(2.0 * math.asin(math.sqrt(math.cos(yy) ** 2 * math.sin((x[k + 1] - x[k]) / 2) ** 2))
                             for k in range(c0[b], c1[b])) * CR.RADIUS
            assert abs(arc.values[a, b] - want) <= 1e-12 * want, (a, b)
