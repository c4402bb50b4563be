"""K10 (xc_clen.hip, xc_contour_lengths) at every launch geometry, on coordinates that differ in every cell, and its fixed-point sum
bit for bit.

Why: longitude only enters a length as x2 - x1 (and, in the Cartesian metric, latitude as y2 - y1), so on an evenly spaced grid a
kernel that reads the coordinates of the wrong column or row gets exactly the right lengths.  Here every spacing is
scale (1 + 0.25 f(i)) with a hashed f, some grids are stretched (widest cell >= 100x the narrowest) and latitude runs downwards.

Every row asserts the record of xc_last_clen_geometry (Context.last_clen_geometry) -- LDS copies, level groups, blocks per slab and
the rule that set them -- then checks the results against the numpy restatement (clength_ref.contour_lengths_fast): counts exact,
NaN pattern exact, totals within 1e-12.  Where every length is exact (tracers that vary along one axis only, spacings of few
significant bits) the totals must equal the fixed-point model clength_ref.det_totals bit for bit.  A level's total must not depend on
the other levels of the call, the launch geometry, shared or per-slab levels, batching or the resident path."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import clength_ref as CR

pytestmark = pytest.mark.gpu

TOL = 1e-12


# ------------------------------------------------------------------------------------------------------------------- launch model
def expected_geometry(N, ny, nx, nslab):
    """the choices of launch_contour_lengths (xc_clen.hip), restated: LDS copies, level groups, tiles, blocks per slab and their rule
    (clength_ref.launch_geometry with K10's 5 words and 32767 cells per LDS copy)"""
    return CR.launch_geometry(N, ny, nx, nslab, words=5, copy_cells=32767)


def run(ctx, q, lv, y, x, latlon, want=None):
    """one call; asserts the launch record against the model (and the pinned fields of `want`) -> (lengths, counts, record)"""
    lens, cnts = ctx.contour_lengths(q, lv, y, x, radius=CR.RADIUS if latlon else 0.0)
    g = ctx.last_clen_geometry()
    S, ny, nx = q.shape
    N = np.shape(lv)[-1]
    exp = expected_geometry(N, ny, nx, S)
    exp.update(q_dtype=np.dtype(q.dtype), latlon=int(latlon))
    for k, v in exp.items():
        assert g[k] == v, 'record %s: %r, expected %r' % (k, g[k], v)
    for k, v in (want or {}).items():
        assert g[k] == v, 'record %s: %r, pinned %r' % (k, g[k], v)
    return lens, cnts.astype(np.int64), g


def reference(planes, index, lv, y, x, latlon):
    """restatement per DISTINCT plane (planes[index[s]] is slab s) -> totals (S, N), counts (S, N)"""
    per_slab = np.ndim(lv) == 2
    cache, tt, nn = {}, [], []
    for s, p in enumerate(index):
        key = (p, s if per_slab else -1)
        if key not in cache:
            cache[key] = CR.contour_lengths_fast(planes[p].astype(np.float64), lv[s] if per_slab else lv, y, x, latlon)
        tt.append(cache[key][0]); nn.append(cache[key][1])
    return np.stack(tt), np.stack(nn)


def check(lens, cnts, rt, rn, what=''):
    assert np.array_equal(cnts, rn), '%s: counts' % what
    assert np.array_equal(np.isnan(lens), np.isnan(rt)), '%s: NaN pattern' % what
    ok = ~np.isnan(rt)
    if ok.any():
        r = np.max(np.abs(lens[ok] - rt[ok]) / np.abs(rt[ok]))
        assert r <= TOL, '%s: rel %.3g' % (what, r)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def bits_equal(a, b):
    return np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------------------------- inputs
def field(ny, nx, seed=0, noise=0.15):
    """a smooth two-scale field plus noise: many closed and open contours, saddles"""
    rng = np.random.default_rng(seed)
    j, i = np.meshgrid(np.linspace(0.0, 1.0, ny), np.linspace(0.0, 1.0, nx), indexing='ij')
    q = np.sin(2.5 * np.pi * j + seed) + 0.6 * np.cos(3.5 * np.pi * i + 0.3 * seed) * np.sin(np.pi * j) + 0.3 * np.sin(9 * i * j)
    return q + noise * rng.standard_normal((ny, nx))


def stretched(n, salt, lo, hi, descending=False):
    """coordinates from lo to hi whose spacings grow geometrically (widest >= 100x narrowest) and differ in every cell"""
    d = np.geomspace(1.0, 300.0, n - 1) * np.diff(CR.hashed_coords(n, salt))
    c = lo + (hi - lo) * np.concatenate([[0.0], np.cumsum(d)]) / np.sum(d)
    return c[::-1].copy() if descending else c


def coords(kind, ny, nx, latlon, salt=0):
    """(y, x) as the library receives them (radians on the sphere)"""
    if kind == 'hashed':
        lat = CR.hashed_coords(ny, salt + 1, -80.0, 160.0 / (ny - 1))
        lon = CR.hashed_coords(nx, salt + 2, 0.0, 350.0 / (nx - 1))
    elif kind == 'stretched':
        lat, lon = stretched(ny, salt + 3, -85.0, 85.0), stretched(nx, salt + 4, 0.0, 355.0)
    else:                                                           # 'descending': latitude 90 -> -90 in uneven steps
        lat = CR.hashed_coords(ny, salt + 5, -89.0, 178.0 / (ny - 1), descending=True)
        lon = CR.hashed_coords(nx, salt + 6, 0.0, 350.0 / (nx - 1))
    if latlon:
        return np.deg2rad(lat), np.deg2rad(lon)
    return lat * 1.1e5, lon * 0.8e5


def levels_in(q, N, seed=0, uniform=False):
    lo, hi = float(np.nanmin(q)), float(np.nanmax(q))
    if uniform:
        return np.linspace(lo, hi, N + 2)[1:-1]
    return np.sort(np.random.default_rng(seed).uniform(lo, hi, N))


# ------------------------------------------------------------------------------------------------------------------- (a) coordinates
A_ROWS = [(kind, latlon, dt, per_slab) for kind in ('hashed', 'stretched', 'descending') for latlon in (False, True)
          for dt in (np.float32, np.float64) for per_slab in (False, True)]


@pytest.mark.parametrize('kind,latlon,dt,per_slab', A_ROWS,
                         ids=['%s-%s-%s-%s' % (k, 'sph' if l else 'cart', np.dtype(d).name, 'slab' if p else 'shared')
                              for k, l, d, p in A_ROWS])
def test_coordinates_that_differ_in_every_cell(ctx, kind, latlon, dt, per_slab):
    ny, nx, S = 67, 131, 3
    planes = [field(ny, nx, seed=s).astype(dt) for s in range(S)]
    q = np.stack(planes)
    y, x = coords(kind, ny, nx, latlon)
    for c in (y, x):
        d = np.abs(np.diff(c))
        assert np.unique(d).size == d.size and (kind != 'stretched' or d.max() >= 100 * d.min())
    assert (np.diff(y) < 0).all() == (kind == 'descending')
    lv = np.stack([levels_in(q[s], 23, seed=s) for s in range(S)]) if per_slab else levels_in(q, 23, uniform=True)
    lens, cnts, _ = run(ctx, q, lv, y, x, latlon, want=dict(ncopy=8, ngroup=1, bps_rule='ntile'))
    rt, rn = reference(planes, range(S), lv, y, x, latlon)
    check(lens, cnts, rt, rn, kind)
    assert (rn > 0).mean() > 0.75


# ------------------------------------------------------------------------------------------------------------------- (b) + (c) geometry
PROBE = np.array([-0.71, -0.2, 0.13, 0.55, 0.9])       # levels that sit inside every set of row b: their bits must not move


def probe_set(N, seed):
    """N ascending levels that contain PROBE: the rest drawn over the field's range"""
    rest = np.random.default_rng(seed).uniform(-1.6, 1.6, N - PROBE.size)
    return np.sort(np.concatenate([PROBE, rest]))


GEOM = [(136, 8, 1), (137, 4, 1), (266, 4, 1), (267, 2, 1), (511, 2, 1), (512, 1, 1), (944, 1, 1), (945, 1, 2), (1889, 1, 3)]


@pytest.fixture(scope='module')
def probe_plane():
    ny, nx = 41, 75
    q = np.stack([field(ny, nx, seed=11), field(ny, nx, seed=12)[::-1]])
    y, x = coords('hashed', ny, nx, False, salt=9)
    return q, y, x


@pytest.fixture(scope='module')
def probe_alone(ctx, probe_plane):
    q, y, x = probe_plane
    lens, cnts, g = run(ctx, q, PROBE, y, x, False, want=dict(ncopy=8))
    check(lens, cnts, *reference(list(q), range(2), PROBE, y, x, False), 'probe alone')
    return lens, cnts


@pytest.mark.parametrize('N,ncopy,ngroup', GEOM, ids=['N%d' % g[0] for g in GEOM])
def test_lds_copies_and_level_groups(ctx, probe_plane, probe_alone, N, ncopy, ngroup):
    q, y, x = probe_plane
    lv = probe_set(N, N)
    lens, cnts, g = run(ctx, q, lv, y, x, False, want=dict(ncopy=ncopy, ngroup=ngroup, G=min(N, 944)))
    check(lens, cnts, *reference(list(q), range(2), lv, y, x, False), 'N=%d' % N)
    at = np.searchsorted(lv, PROBE)
    assert bits_equal(lens[:, at], probe_alone[0]) and np.array_equal(cnts[:, at], probe_alone[1])
    # per-slab levels (the second slab's set differs), across the group split where there is one
    lv2 = np.stack([lv, probe_set(N, N + 1)])
    l2, c2, _ = run(ctx, q, lv2, y, x, False, want=dict(ncopy=ncopy, ngroup=ngroup))
    check(l2, c2, *reference(list(q), range(2), lv2, y, x, False), 'N=%d per slab' % N)
    assert bits_equal(l2[0], lens[0]) and np.array_equal(c2[0], cnts[0])
    at2 = np.searchsorted(lv2[1], PROBE)
    assert bits_equal(l2[1, at2], probe_alone[0][1])


def test_trailing_inf_levels_and_shared_vs_per_slab_and_batches_and_resident(ctx, probe_plane, probe_alone):
    q, y, x = probe_plane
    lv = np.concatenate([PROBE, [np.inf, np.inf]])                        # what the facade makes of NaN levels
    lens, cnts, _ = run(ctx, q, lv, y, x, False)
    assert np.isnan(lens[:, -2:]).all() and (cnts[:, -2:] == 0).all()
    assert bits_equal(lens[:, :-2], probe_alone[0]) and np.array_equal(cnts[:, :-2], probe_alone[1])
    l2, _, _ = run(ctx, q, np.stack([PROBE, PROBE]), y, x, False)
    assert bits_equal(l2, probe_alone[0])
    big = np.concatenate([q, q[::-1], q])                                 # six slabs, then three batches of two
    whole, _, _ = run(ctx, big, PROBE, y, x, False)
    old = ctx.max_batch_bytes
    try:
        ctx.max_batch_bytes = 2 * q[0].nbytes
        split, _ = ctx.contour_lengths(big, PROBE, y, x)
        assert ctx.last_clen_geometry()['nslab'] == 2
    finally:
        ctx.max_batch_bytes = old
    assert bits_equal(split, whole) and bits_equal(whole[:2], probe_alone[0]) and bits_equal(whole[2], probe_alone[0][1])
    ctx.keep_resident(big)
    try:
        res, _ = ctx.contour_lengths(big, PROBE, y, x)
        assert ctx.resident_ptr(big)
    finally:
        ctx.release_resident(big)
    assert bits_equal(res, whole)


def _stack(planes, index, dt):
    return np.stack([planes[p] for p in index]).astype(dt)


@pytest.mark.parametrize('rule,S,ny,nx,N', [
    ('share', 64, 545, 254, 40),        # ntile 17 x 2 = 34 > share 32 > need 2
    ('floor', 300, 289, 101, 40),       # share 6 -> 8 < ntile 9; need 1
    ('capacity', 256, 961, 2, 600),     # one copy: max_tiles 3, ntile 30 -> need 10 > share 8
    ('ntile', 1, 33, 64, 40),
])
def test_blocks_per_slab_rules(ctx, rule, S, ny, nx, N):
    planes = [field(ny, nx, seed=20 + p, noise=0.3) for p in range(4)]
    index = [(s * 7) % 4 for s in range(S)]                                # four distinct slabs, repeated
    q = _stack(planes, index, np.float32)
    y, x = coords('hashed', ny, nx, False, salt=3)
    lv = levels_in(q[:4], N, seed=1)
    lens, cnts, g = run(ctx, q, lv, y, x, False, want=dict(bps_rule=rule))
    check(lens, cnts, *reference([p.astype(np.float32) for p in planes], index, lv, y, x, False), rule)
    # the same slabs alone: another bps, the same bits
    if S > 4:
        one, _, g1 = run(ctx, q[:4], lv, y, x, False)
        assert g1['bps'] != g['bps'] and bits_equal(one, lens[:4])


EDGE_X = [1, 62, 63, 64, 251, 252, 253, 504, 505]
EDGE_Y = [1, 3, 4, 5, 31, 32, 33]


@pytest.mark.parametrize('ncy', EDGE_Y)
def test_tile_and_wave_edges(ctx, ncy):
    """nx - 1 across the wave (63 cells) and tile (252) boundaries, ny - 1 across the row batches (4) and tiles (32)"""
    for ncx in EDGE_X:
        ny, nx = ncy + 1, ncx + 1
        planes = [field(ny, nx, seed=ncx + ncy, noise=0.4), field(ny, nx, seed=ncx * ncy + 1, noise=0.4)]
        q = np.stack(planes)
        y, x = coords('descending', ny, nx, True, salt=ncx)
        lv = levels_in(q, 17, seed=ncx)
        lens, cnts, _ = run(ctx, q, lv, y, x, True, want=dict(ntile=-(-ncy // 32) * -(-ncx // 252)))
        check(lens, cnts, *reference(planes, range(2), lv, y, x, True), 'cells %dx%d' % (ncy, ncx))


@pytest.mark.parametrize('shape', [(1, 40), (30, 1), (1, 1)])
def test_planes_without_cells(ctx, shape):
    ny, nx = shape
    q = np.random.default_rng(0).standard_normal((3, ny, nx))
    lens, cnts, g = run(ctx, q, [-0.5, 0.0, 0.5], np.arange(ny) * 1.5, np.arange(nx) * 0.5, False,
                        want=dict(ntile=0, bps=0, bps_rule=None))
    assert np.isnan(lens).all() and (cnts == 0).all()


def test_checkerboard_saturates_every_copy(ctx):
    """every cell a saddle across every level: each block of the capacity-bound launch gives its one LDS copy three full tiles
    (24192 cells, 2 segments per level each) -- close to the 32767-cell budget.  Corners +-1 and levels -1 + 2m/1024 make every
    end point exact on unit spacing: each segment is hypot(g, g) with g = (1 - c) / 2"""
    ny, nx, S = 32 * 27 + 1, 253, 256                                      # ntile 27, need 9 > share 8
    cb = np.where(np.indices((ny, nx)).sum(0) % 2 == 0, 1.0, -1.0).astype(np.float32)
    q = np.zeros((S, ny, nx), dtype=np.float32)
    q[0] = cb; q[S - 1] = -cb                                              # two saturated slabs, the others flat
    lv = -1.0 + 2.0 * np.arange(300, 300 + 600) / 1024.0
    lens, cnts, g = run(ctx, q, lv, np.arange(float(ny)), np.arange(float(nx)), False,
                        want=dict(ncopy=1, ngroup=1, bps=9, bps_rule='capacity'))
    ncell = (ny - 1) * (nx - 1)
    assert (cnts[[0, S - 1]] == 2 * ncell).all() and (cnts[1:S - 1] == 0).all() and np.isnan(lens[1:S - 1]).all()
    gg = (1.0 - lv) / 2.0
    want = 2 * ncell * np.hypot(gg, gg)
    for s in (0, S - 1):
        assert np.max(np.abs(lens[s] - want) / want) <= TOL


# ------------------------------------------------------------------------------------------------------------------- (d) fixed point
few_bits = CR.few_bits              # (shared with the K11 geometry tests)


FP_ROWS = ['x-only', 'y-only', 'wide-column', 'wide-row', 'tall-cells']


@pytest.mark.parametrize('row', FP_ROWS)
def test_fixed_point_rule_bit_for_bit(ctx, row):
    """Segments along one axis only: every length is one spacing, exactly (premise: hypot(0, d) == |d| on the device, d of <= 26
    significant bits), so the totals must be the fixed-point model det_totals bit for bit.  'wide-*': one cell 2^160 times the others
    lifts the window top and the short segments lose their low chunks into the trash word -- the model drops the same bits, np.sum
    does not.  'tall-cells': dy ~ 1e4 dx, the y spacing sets the window bound
    (segments of 2^14 and more would overflow a window set by dx alone)."""
    ny, nx = 97, 301
    y, x = few_bits(ny, 1, 1.0), few_bits(nx, 2, 1.0)
    if row == 'wide-column':                                                 # window 2^133 .. 2^-59; segments ~2^-40, bits to 2^-61
        y = few_bits(ny, 1, 2.0 ** -40)
        x[150:] += 2.0 ** 120
    if row == 'wide-row':
        x = few_bits(nx, 2, 2.0 ** -40)
        y[50:] += 2.0 ** 120
    if row == 'tall-cells':                                                  # dy up to ~2e4 dx: above 2^14, past what dx alone bounds
        y = few_bits(ny, 3, 2.0 ** 14)
    along_x = row in ('x-only', 'wide-column', 'tall-cells')
    rng = np.random.default_rng(len(row))
    prof = np.sort(rng.uniform(-3.0, 3.0, nx if along_x else ny))
    prof[::17] = prof[1::17][:prof[::17].size]                               # some flat sides: levels on two equal nodes
    plane = np.broadcast_to(prof[None, :] if along_x else prof[:, None], (ny, nx))
    q = np.stack([plane, plane[::-1, ::-1]]).astype(np.float64)
    lv = np.concatenate([np.sort(rng.uniform(-3.2, 3.2, 30)), prof[[5, 40, 77]]])
    lv.sort()
    lens, cnts, _ = run(ctx, q, lv, y, x, False)
    ref = reference(list(q), range(2), lv, y, x, False)
    assert np.array_equal(cnts, ref[1])
    model = np.stack([CR.det_totals(q[s], lv, y, x, False) for s in range(2)])
    assert np.array_equal(np.isnan(lens), np.isnan(model))
    assert bits_equal(lens, model), 'fixed-point rule: max ulp %d' % np.max(np.abs(bits(lens) - bits(model)))
    if row.startswith('wide'):
        assert not bits_equal(model, ref[0]), 'the wide cell must cost the short segments bits'
    else:
        check(lens, cnts, *ref, row)


# ------------------------------------------------------------------------------------------------------------------- (e) level search
def on_and_next_to(q, lv, rng, dt):
    """corners exactly on a level and one ulp (of the tracer dtype) to either side"""
    S, ny, nx = q.shape
    for s in range(S):
        j, i = rng.integers(0, ny, 300), rng.integers(0, nx, 300)
        v = dt(lv[rng.integers(0, lv.size, 300)])
        q[s, j, i] = np.where(np.arange(300) % 3 == 0, v, np.where(np.arange(300) % 3 == 1, np.nextafter(v, dt(np.inf)),
                                                                     np.nextafter(v, dt(-np.inf))))
    return q


@pytest.mark.parametrize('latlon', [False, True])
@pytest.mark.parametrize('dt', [np.float32, np.float64])
@pytest.mark.parametrize('kind', ['f32-linspace-300', 'f32-linspace-1e-4', 'duplicated'])
def test_equally_spaced_search_edges(ctx, kind, dt, latlon):
    rng = np.random.default_rng(len(kind))
    ny, nx = 53, 97
    if kind == 'f32-linspace-300':
        lv = np.linspace(299.0, 301.0, 41).astype(np.float32).astype(np.float64)
        base = 300.0 + 1.2 * np.stack([field(ny, nx, seed=1), field(ny, nx, seed=2)]) / 1.5
    elif kind == 'f32-linspace-1e-4':
        lv = np.linspace(-1e-4, 1e-4, 33).astype(np.float32).astype(np.float64)
        base = 1.1e-4 * np.stack([field(ny, nx, seed=3), field(ny, nx, seed=4)]) / 1.5
    else:
        lv = np.sort(np.concatenate([np.linspace(-1.0, 1.0, 21), [-0.5, 0.3, 0.3]]))
        base = np.stack([field(ny, nx, seed=5), field(ny, nx, seed=6)])
    q = on_and_next_to(base.astype(dt), lv, rng, dt)
    y, x = coords('hashed', ny, nx, latlon, salt=4)
    lens, cnts, _ = run(ctx, q, lv, y, x, latlon)
    check(lens, cnts, *reference(list(q), range(2), lv, y, x, latlon), kind)
    if kind == 'duplicated':
        d = np.nonzero(np.diff(lv) == 0)[0]
        assert bits_equal(lens[:, d], lens[:, d + 1])


# ------------------------------------------------------------------------------------------------------------------- (f) non-finite
@pytest.mark.parametrize('latlon', [False, True])
def test_infinite_corners(ctx, latlon):
    ny, nx = 45, 80
    q = np.stack([field(ny, nx, seed=7), field(ny, nx, seed=8)])
    # slab 0: +inf and -inf in corner cells of the plane: a level crosses the infinite corner's edges (NaN end points, so a NaN
    # total through the flag) or only the finite ones (a finite total) -- both happen
    q[0, :2, :2] = [[np.inf, 1.0], [1.0, -1.0]]
    q[0, -2:, -2:] = [[1.2, -0.4], [-0.4, -np.inf]]
    # slab 1: infinities inside the plane, next to a NaN
    q[1, 10, 20] = np.inf; q[1, 30, 5] = -np.inf; q[1, 30, 6] = np.inf
    q[1, 3, 70] = np.inf; q[1, 40, 40] = np.nan; q[1, 41, 41] = -np.inf
    y, x = coords('stretched', ny, nx, latlon, salt=2)
    lv = np.linspace(-1.5, 1.5, 29)
    lens, cnts, _ = run(ctx, q, lv, y, x, latlon)
    rt, rn = reference(list(q), range(2), lv, y, x, latlon)
    check(lens, cnts, rt, rn, 'inf corners')
    assert np.isnan(rt[0, 1:-1]).sum() >= 3 and (~np.isnan(rt[0])).sum() >= 10     # both outcomes are reached


# ------------------------------------------------------------------------------------------------------------------- (g) facade
def test_facade_descending_uneven_float32_coordinates_and_transpose(ctx):
    import xcontour_amd as xa
    ny, nx = 73, 144
    lat = CR.hashed_coords(ny, 12, -88.0, 176.0 / (ny - 1), descending=True).astype(np.float32)
    lon = stretched(nx, 13, 0.0, 357.5).astype(np.float32)
    q = np.stack([field(ny, nx, seed=s) for s in range(2)])
    lv = np.array([0.4, -1.1, np.nan, 0.05, 1.3, -0.6])

    def facade(arr, dims):
        c = {'lat': lat, 'lon': lon, 'time': np.arange(2)}
        tr = xa.DataArray(arr, dims, {d: c[d] for d in dims}, 'q')
        return xa.Contour2D(tr, np.ones(ny), {'X': 'lon', 'Y': 'lat'}, {'Y': 'lat'}, dtype=np.float64)

    got = facade(q, ('time', 'lat', 'lon')).cal_contour_lengths(lv, latlon=True).values
    y, x = CR.plane_coords(lat, lon, True)
    for s in range(2):
        rt, _ = CR.contour_lengths_fast(q[s], lv, y, x, True)
        assert np.array_equal(np.isnan(got[s]), np.isnan(rt))
        ok = ~np.isnan(rt)
        assert np.max(np.abs(got[s][ok] - rt[ok]) / rt[ok]) <= TOL
    tr = facade(np.ascontiguousarray(q.transpose(0, 2, 1)), ('time', 'lon', 'lat')).cal_contour_lengths(lv, latlon=True).values
    assert bits_equal(tr, got)


# ------------------------------------------------------------------------------------------------------------------- (h) completeness
# instantiation -> the rows that reach it (and assert it through the record: q_dtype, latlon)
ROWS = {('f32', False): 'test_coordinates_that_differ_in_every_cell[*-cart-float32-*], test_blocks_per_slab_rules',
        ('f64', False): 'test_coordinates_that_differ_in_every_cell[*-cart-float64-*], test_fixed_point_rule_bit_for_bit',
        ('f32', True): 'test_coordinates_that_differ_in_every_cell[*-sph-float32-*], test_equally_spaced_search_edges',
        ('f64', True): 'test_coordinates_that_differ_in_every_cell[*-sph-float64-*], test_tile_and_wave_edges',
        'window': 'every row (k_clen_window)', 'finish': 'every row (k_clen_finish)'}


def parse_symbol(s):
    m = re.search(r'6k_clenI([df])Lb([01])EE', s)
    if m:
        return ({'d': 'f64', 'f': 'f32'}[m.group(1)], m.group(2) == '1')
    for k in ('window', 'finish'):
        if 'k_clen_' + k in s:
            return k
    raise AssertionError('unrecognised K10 kernel symbol %s' % s)


def test_every_instantiation_has_a_row(tmp_path):
    """every k_clen* kernel of the gfx950 code object has a row here, and every row names one that exists.  Runs no kernel."""
    from xcontour_amd import _native as nat
    tool = '/opt/rocm/llvm/bin'
    lib = str(tmp_path / 'lib.so')
    shutil.copy(nat.LIB_PATH, lib)
    subprocess.run([os.path.join(tool, 'llvm-objdump'), '--offloading', lib], check=True, cwd=str(tmp_path), stdout=subprocess.DEVNULL)
    syms = set()
    for f in sorted(os.listdir(str(tmp_path))):
        if 'gfx950' in f:
            out = subprocess.run([os.path.join(tool, 'llvm-readelf'), '-Ws', str(tmp_path / f)], check=True, stdout=subprocess.PIPE,
                                 universal_newlines=True).stdout
            syms |= set(m for m in re.findall(r'\b(_Z\S*k_clen\S*)', out) if '.' not in m)
    keys = set(parse_symbol(s) for s in syms)
    assert len(keys) == len(syms) == 6
    assert keys == set(ROWS), 'instantiations without a row: %s; rows without one: %s' % (keys - set(ROWS), set(ROWS) - keys)
    assert {(np.dtype(d).name.replace('float', 'f'), bool(l)) for _, l, d, _ in A_ROWS} == {k for k in ROWS if isinstance(k, tuple)}
