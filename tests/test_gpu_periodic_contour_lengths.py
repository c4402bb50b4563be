"""The periodic X direction of K10 / K11 (xc_contour_lengths_periodic, xc_local_contour_lengths_periodic; `periodic=` of
Contour2D.cal_contour_lengths / cal_local_contour_lengths) on the GPU.

Identity: on dyadic coordinates with a dyadic period (x +/- period is exact, the window constant identical) the periodic call equals,
bit for bit, the shipped non-periodic kernel on the plane with the ring's columns copied beside it (clength_periodic_ref.extend_plane
for K10, tile_plane for K11).  Independently: against the numpy restatement on hashed coordinates -- counts exact, totals within
1e-12, NaN where it has NaN, the bounds of the K10 / K11 tests against the same restatement.  And the bits do not depend on slabs per
call, batching, the resident path or (K11) the stride; period=None is the old entry point."""
import numpy as np
import pytest

import clength_periodic_ref as PR
import clength_ref as CR
import local_clength_ref as LR
import xcontour_amd as xa
from xcontour_amd import _native as nat

pytestmark = pytest.mark.gpu


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def check(lens, cnts, ref_t, ref_n, what=''):
    lens, cnts = np.asarray(lens), np.asarray(cnts).astype(np.int64)
    assert np.array_equal(cnts, ref_n), what
    assert np.array_equal(np.isnan(lens), np.isnan(ref_t)), what
    ok = ~np.isnan(ref_t)
    if ok.any():
        r = np.abs(lens[ok] - ref_t[ok]) / np.abs(ref_t[ok])
        assert r.max() <= 1e-12, '%s: rel %.3g' % (what, r.max())


def field(kind, shape, seed, dt=np.float64):
    rng = np.random.default_rng(seed)
    ny, nx = shape[-2:]
    if kind == 'saddle':
        q = np.indices((ny, nx)).sum(0) % 2 * 2.0 - 1.0 + 0.3 * rng.standard_normal(shape)    # checkerboard: saddles in the seam cell too
    elif kind == 'node':
        q = rng.integers(0, 6, size=shape).astype(np.float64)                                  # levels fall on node values
    else:
        q = rng.standard_normal(shape)
    if kind == 'nan':
        q[rng.random(shape) < 0.08] = np.nan
        q[..., ny // 2, 0] = np.nan                                                            # some of them beside the seam
        q[..., ny - 1, nx - 1] = np.nan
    return q.astype(dt)


def levels_for(kind, ns, n, seed):
    """per-slab ascending levels (ns, n)"""
    if kind == 'node':
        pool = np.array([-1.0, 0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 4.0, 4.5, 5.0, 6.0])
        rng = np.random.default_rng(seed)
        return np.stack([np.sort(rng.choice(pool, size=min(n, pool.size), replace=False)) for _ in range(ns)])
    return np.sort(np.random.default_rng(seed).uniform(-1.5, 1.5, (ns, n)), axis=1)


def dyadic(n, salt, unit, start=0.0, descending=False):
    """n coordinates whose spacings are 1, 2, 3 or 4 x unit (a power of two), differing from cell to cell"""
    i = np.arange(max(n - 1, 0), dtype=np.int64)
    d = ((i * 7 + salt * 3 + (i >> 2)) % 4 + 1) * unit
    c = start + np.concatenate([[0.0], np.cumsum(d)])
    return -c if descending else c


def dyadic_plane(ny, nx, latlon):
    """-> (y, x, period): every value a small multiple of a power of two, so x +/- period is exact; the seam cell is 3 units wide.
    Sphere: latitude descending within (-pi/2, pi/2), longitude below 2 pi + a little (radians need not be a real globe)."""
    if latlon:
        y = dyadic(ny, 1, 2.0 ** -6, start=-1.25, descending=True)             # 1.25 ... >= 1.25 - 33 * 4 / 64 = -0.81
        x = dyadic(nx, 2, 2.0 ** -9)                                            # <= 504 * 4 / 512 = 3.94
        return y, x, float(x[-1] - x[0] + 3 * 2.0 ** -9)
    y, x = dyadic(ny, 3, 0.5, start=5.0), dyadic(nx, 4, 0.25, start=-3.0)
    return y, x, float(x[-1] - x[0] + 0.75)


def hashed_plane(ny, nx, latlon):
    """coordinates whose spacings differ in every cell (latitude descending on the sphere) and a period that is no sum of theirs"""
    if latlon:
        y = np.deg2rad(CR.hashed_coords(ny, 1, -80.0, 160.0 / ny, descending=True))
        x = np.deg2rad(CR.hashed_coords(nx, 2, 0.0, 300.0 / nx))
        return y, x, 2.0 * np.pi
    y, x = CR.hashed_coords(ny, 3, 5.0, 7.0), CR.hashed_coords(nx, 4, -3.0, 2.0)
    return y, x, float(x[-1] - x[0]) + 1.7


# ================================================================== K10
K10_NX = (2, 3, 64, 65, 252, 253, 254, 505)       # 252: the seam cell is the last cell of the first tile column; 253: the only cell of the
K10_NY = (2, 33, 34)                              # second; 64 / 65: on a wave edge.  33 / 34: one tile row and one cell row more


@pytest.mark.parametrize('kind', ['random', 'saddle', 'node', 'nan'])
@pytest.mark.parametrize('latlon', [False, True])
@pytest.mark.parametrize('dt', [np.float32, np.float64])
def test_k10_periodic_is_the_shipped_kernel_on_the_extended_plane(ctx, dt, latlon, kind):
    radius = CR.RADIUS if latlon else 0.0
    nseg = 0
    for nx in K10_NX:
        for ny in K10_NY:
            q = field(kind, (2, ny, nx), 100 * nx + ny, dt)
            y, x, period = dyadic_plane(ny, nx, latlon)
            lv = levels_for(kind, 2, 9, nx + ny)
            qe, xe = PR.extend_plane(q, x, period)
            assert xe[-1] - period == x[0]                                      # the addition was exact
            a, na = ctx.contour_lengths(q, lv, y, x, radius=radius, period=period)
            g = ctx.last_clen_geometry()
            assert g['ntile'] == -(-(ny - 1) // 32) * -(-nx // 252), (nx, ny)  # tiles over nx cell columns (253: a second tile column)
            assert g['latlon'] == int(latlon) and g['q_dtype'] == np.dtype(dt)
            b, nb = ctx.contour_lengths(np.ascontiguousarray(qe), lv, y, xe, radius=radius)
            assert np.array_equal(na, nb), (nx, ny)
            assert bits_equal(a, b), (nx, ny)
            nseg += int(na.sum())
    assert nseg > 0


def test_k10_periodic_two_level_groups(ctx):
    ny, nx, N = 34, 253, 2000                                                   # more levels than one LDS pass takes
    q = field('random', (2, ny, nx), 5)
    y, x, period = dyadic_plane(ny, nx, False)
    lv = np.sort(np.random.default_rng(6).uniform(-3.0, 3.0, N))
    a, na = ctx.contour_lengths(q, lv, y, x, period=period)
    assert ctx.last_clen_geometry()['ngroup'] >= 2
    qe, xe = PR.extend_plane(q, x, period)
    b, nb = ctx.contour_lengths(np.ascontiguousarray(qe), lv, y, xe)
    assert np.array_equal(na, nb) and bits_equal(a, b) and na.sum() > 0


@pytest.mark.parametrize('latlon', [False, True])
@pytest.mark.parametrize('kind', ['random', 'saddle', 'node', 'nan'])
def test_k10_periodic_matches_restatement(ctx, kind, latlon):
    for ny, nx in ((2, 2), (5, 3), (9, 253), (34, 65)):
        q = field(kind, (2, ny, nx), 7 + nx)
        y, x, period = hashed_plane(ny, nx, latlon)
        lv = levels_for(kind, 2, 9, 3)
        lens, cnts = ctx.contour_lengths(q, lv, y, x, radius=CR.RADIUS if latlon else 0.0, period=period)
        for s in range(2):
            rt, rn = PR.contour_lengths(q[s], lv[s], y, x, period, latlon)
            check(lens[s], cnts[s], rt, rn, '%s %dx%d latlon=%s slab %d' % (kind, ny, nx, latlon, s))
    # a descending X coordinate and its negative period: the same ring walked the other way
    lens2, cnts2 = ctx.contour_lengths(np.ascontiguousarray(q[..., ::-1]), lv, y, x[::-1].copy(), radius=CR.RADIUS if latlon else 0.0,
                                       period=-period)
    assert np.array_equal(cnts2, cnts)
    ok = ~np.isnan(lens)
    assert np.array_equal(np.isnan(lens2), ~ok) and (not ok.any() or np.max(np.abs(lens2[ok] - lens[ok]) / lens[ok]) <= 1e-12)


def test_k10_closed_ring(ctx):
    """q = f(row): every level between two rows is one closed line of length |period| exactly (dyadic Cartesian ring)"""
    ny, nx = 9, 300
    q = np.repeat((np.arange(ny, dtype=np.float64) * 3.0)[:, None], nx, axis=1)
    y, x, period = dyadic_plane(ny, nx, False)
    lv = np.array([0.7, 10.1, 22.5])
    lens, cnts = ctx.contour_lengths(q[None], lv, y, x, period=period)
    assert np.array_equal(lens[0], np.full(3, period)) and np.array_equal(cnts[0], np.full(3, nx))
    lens, cnts = ctx.contour_lengths(q[None], lv, y, x)
    assert np.array_equal(lens[0], np.full(3, period - 0.75)) and np.array_equal(cnts[0], np.full(3, nx - 1))


def _raw_k10(ctx, name, q, lv, y, x, radius, period=None):
    """the C entry point `name` called directly"""
    ns, ny, nx = q.shape
    lens, cnts = np.empty((ns, lv.shape[-1])), np.empty((ns, lv.shape[-1]), dtype=np.uint64)
    mid = (radius,) if period is None else (period, radius)
    ctx._check(getattr(ctx.lib, name)(ctx.handle, nat._ptr(q), nat.dtype_code(q.dtype), ns, ny, nx, nat._ptr(y), nat._ptr(x), *mid,
                                      nat._ptr(lv), lv.shape[-1], 1 if lv.ndim == 2 else 0, nat._ptr(lens), nat._ptr(cnts)))
    return lens, cnts


def _raw_k11(ctx, name, q, y, x, radius, window, stride, mp, period=None):
    ns, ny, nx = q.shape
    nw = (-(-ny // stride[0]), -(-nx // stride[1]))
    lens, lvls, cnts = np.empty((ns,) + nw), np.empty((ns,) + nw), np.empty((ns,) + nw, dtype=np.uint64)
    mid = (radius,) if period is None else (period, radius)
    ctx._check(getattr(ctx.lib, name)(ctx.handle, nat._ptr(q), nat.dtype_code(q.dtype), ns, ny, nx, nat._ptr(y), nat._ptr(x), *mid,
                                      window[0], window[1], stride[0], stride[1], mp, None, nat._ptr(lens), nat._ptr(lvls), nat._ptr(cnts)))
    return lens, lvls, cnts


@pytest.mark.parametrize('latlon', [False, True])
def test_default_is_the_old_entry_point(ctx, latlon):
    """period=None goes through the old symbols and returns their bits; the new symbols, called beside them on the same inputs, add
    the seam cells and nothing else"""
    ny, nx = 34, 130
    q = field('nan', (2, ny, nx), 41)
    y, x, period = hashed_plane(ny, nx, latlon)
    radius = CR.RADIUS if latlon else 0.0
    lv = levels_for('nan', 2, 11, 8)
    old = _raw_k10(ctx, 'xc_contour_lengths', q, lv, y, x, radius)
    new = _raw_k10(ctx, 'xc_contour_lengths_periodic', q, lv, y, x, radius, period)
    dflt = ctx.contour_lengths(q, lv, y, x, radius=radius)
    per = ctx.contour_lengths(q, lv, y, x, radius=radius, period=period)
    assert bits_equal(dflt[0], old[0]) and np.array_equal(dflt[1], old[1])
    assert bits_equal(per[0], new[0]) and np.array_equal(per[1], new[1])
    for s in range(2):
        check(old[0][s], old[1][s], *CR.contour_lengths(q[s], lv[s], y, x, latlon), what='old symbol')
    assert (new[1] >= old[1]).all() and (new[1] > old[1]).any()
    window, stride = (7, 9), (3, 4)
    old = _raw_k11(ctx, 'xc_local_contour_lengths', q, y, x, radius, window, stride, 1)
    new = _raw_k11(ctx, 'xc_local_contour_lengths_periodic', q, y, x, radius, window, stride, 1, period)
    dflt = ctx.local_contour_lengths(q, y, x, window, stride, 1, radius=radius)
    per = ctx.local_contour_lengths(q, y, x, window, stride, 1, radius=radius, period=period)
    for u, v in zip(dflt, old):
        assert bits_equal(u.astype(np.float64), v.astype(np.float64))
    for u, v in zip(per, new):
        assert bits_equal(u.astype(np.float64), v.astype(np.float64))
    for s in range(2):
        assert bits_equal(old[1][s], LR.window_levels(q[s], window, stride, 1))
    inner = slice(2, -3)                                                        # windows that touch no X edge: the same either way
    for u, v in zip(old, new):
        assert bits_equal(u[:, :, inner].astype(np.float64), v[:, :, inner].astype(np.float64))
    assert not bits_equal(old[1][:, :, 0], new[1][:, :, 0])


# ================================================================== K11
def _k11_identity(ctx, q, y, x, period, window, stride, mp, radius, levels=None):
    """the periodic call against the shipped K11 on tile_plane at the matching centres"""
    ns, ny, nx = q.shape
    sx = stride[1]
    h = PR.halo(window[1], sx)
    qt, xt = PR.tile_plane(q, x, period, h)
    assert np.array_equal(xt[h:h + nx], x) and xt[h - 1] + period == x[-1] and xt[h + nx] - period == x[0]      # exact
    a, nwx = h // sx, -(-nx // sx)
    lt = None
    if levels is not None:
        lt = np.zeros(levels.shape[:2] + (-(-(nx + 2 * h) // sx),))
        lt[:, :, a:a + nwx] = levels
    got = ctx.local_contour_lengths(q, y, x, window, stride, mp, levels=levels, radius=radius, period=period)
    ref = ctx.local_contour_lengths(np.ascontiguousarray(qt), y, xt, window, stride, mp, levels=lt, radius=radius)
    what = (nx, window, stride, mp, levels is not None)
    assert got[0].shape == (ns, -(-ny // stride[0]), nwx), what
    assert bits_equal(got[1], ref[1][:, :, a:a + nwx]), what                     # levels
    assert np.array_equal(got[2], ref[2][:, :, a:a + nwx]), what                 # counts
    assert bits_equal(got[0], ref[0][:, :, a:a + nwx]), what                     # lengths
    return got


@pytest.mark.parametrize('latlon', [False, True])
@pytest.mark.parametrize('dt', [np.float32, np.float64])
def test_k11_periodic_is_the_shipped_kernel_on_the_tiled_plane(ctx, dt, latlon):
    radius = CR.RADIUS if latlon else 0.0
    ny, nseg, nnan = 13, 0, 0
    rng = np.random.default_rng(19)
    for nx in (8, 64, 65, 130):
        q = field('nan', (2, ny, nx), nx, dt)
        y, x, period = dyadic_plane(ny, nx, latlon)
        for window in ((7, 9), (6, 4), (5, nx)):
            if window[1] > nx:                                                  # (7, 9) on the ring of 8: wider than the ring
                with pytest.raises(nat.XContourHipError) as e:
                    ctx.local_contour_lengths(q, y, x, window, (3, 4), 1, radius=radius, period=period)
                assert e.value.code == nat.XC_EBADARG and 'wider than the ring' in str(e.value)
                continue
            for stride in ((3, 4), (1, 1)):
                full = window[0] * window[1]
                # means: min_periods below a full window (the NaNs beside the seam and the Y edges decide), then the full window
                for mp in (full - 2 * window[1] - 1, full):
                    got = _k11_identity(ctx, q, y, x, period, window, stride, max(mp, 1), radius)
                    nnan += int(np.isnan(got[1]).sum())
                    nseg += int(got[2].sum())
                nw = got[0].shape[1:]
                given = rng.uniform(-1.0, 1.0, (2,) + nw)
                given[0, 0, 0] = np.nan
                got = _k11_identity(ctx, q, y, x, period, window, stride, 1, radius, levels=given)
                assert bits_equal(got[1], given)
                nseg += int(got[2].sum())
    assert nseg > 0 and nnan > 0


@pytest.mark.parametrize('latlon', [False, True])
@pytest.mark.parametrize('kind', ['random', 'saddle', 'node', 'nan'])
def test_k11_periodic_matches_restatement(ctx, kind, latlon):
    ny, nx, ns = 23, 37, 2
    q = field(kind, (ns, ny, nx), 5 + len(kind))
    y, x, period = hashed_plane(ny, nx, latlon)
    radius = CR.RADIUS if latlon else 0.0
    for window, stride in (((9, 12), (4, 5)), ((6, 37), (5, 9))):
        lens, lvls, cnts = ctx.local_contour_lengths(q, y, x, window, stride, 1, radius=radius, period=period)
        assert cnts.sum() > 0
        for s in range(ns):
            assert bits_equal(lvls[s], PR.window_levels(q[s], window, stride, period, 1)), (window, s)
            rt, rn = PR.local_contour_lengths(q[s], lvls[s], y, x, period, window, stride, latlon)
            check(lens[s], cnts[s], rt, rn, '%s %r latlon=%s slab %d' % (kind, window, latlon, s))


def test_k11_every_window_has_its_full_width(ctx):
    ny, nx, w, s = 40, 48, 9, 1
    q = np.repeat((np.arange(ny, dtype=np.float64) ** 1.5)[:, None], nx, axis=1)
    y, x = np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64)
    lens, lvls, cnts = ctx.local_contour_lengths(q[None], y, x, (w, w), (4, s), 1, period=float(nx))
    assert np.array_equal(lens[0], np.full(lens[0].shape, w - 1.0)) and np.array_equal(cnts[0], np.full(cnts[0].shape, w - 1))
    lens, _, _ = ctx.local_contour_lengths(q[None], y, x, (w, w), (4, s), 1)
    assert lens[0, 0, 0] == w // 2 and lens[0, 0, -1] == w // 2 - 1 + w % 2     # today's seam stripe


# ================================================================== stability of bits
def test_bits_do_not_depend_on_slabs_batches_residency_or_stride(ctx):
    ny, nx, ns = 45, 96, 5
    q = field('nan', (ns, ny, nx), 33)
    lat, lon = np.linspace(-66.0, 66.0, ny), np.arange(nx) * 3.75
    y, x = CR.plane_coords(lat, lon, True)
    period = float(np.float64(np.deg2rad(np.float32(360.0))))
    ctr = np.sort(np.random.default_rng(5).uniform(-2.0, 2.0, (ns, 23)), axis=1)
    kw = dict(radius=CR.RADIUS, period=period)
    a = ctx.contour_lengths(q, ctr, y, x, **kw)
    window = (15, 21)
    b = ctx.local_contour_lengths(q, y, x, window, (5, 4), 100, **kw)
    assert a[1].sum() > 0 and np.nansum(b[2]) > 0
    b2 = ctx.local_contour_lengths(q, y, x, window, (10, 8), 100, **kw)         # every other window of stride (5, 4)
    for u, v in zip(b, b2):
        assert bits_equal(u[:, ::2, ::2].astype(np.float64), v.astype(np.float64))
    for s in range(ns):                                                         # one slab per call
        one = ctx.contour_lengths(q[s:s + 1], ctr[s], y, x, **kw)
        assert bits_equal(one[0][0], a[0][s]) and np.array_equal(one[1][0], a[1][s])
        one = ctx.local_contour_lengths(q[s:s + 1], y, x, window, (5, 4), 100, **kw)
        assert all(bits_equal(u[0].astype(np.float64), v[s].astype(np.float64)) for u, v in zip(one, b))
    old = ctx.max_batch_bytes
    try:
        for nb in (1, 2, 3):                                                    # batches of 1, 2 and 3 slabs
            ctx.max_batch_bytes = nb * ny * nx * 8 + 8
            assert len(ctx._batches(ns, ny * nx * 8)) == -(-ns // nb)
            c = ctx.contour_lengths(q, ctr, y, x, **kw)
            assert bits_equal(c[0], a[0]) and np.array_equal(c[1], a[1]), nb
            ctx.max_batch_bytes = nb * (ny * nx * 8 + 4 * b[0][0].size * 8) + 8
            c = ctx.local_contour_lengths(q, y, x, window, (5, 4), 100, **kw)
            assert all(bits_equal(u.astype(np.float64), v.astype(np.float64)) for u, v in zip(c, b)), nb
    finally:
        ctx.max_batch_bytes = old
    # the facade: a resident object (device mirror, _dev entry points) against numpy-in
    tr = xa.DataArray(q, ('time', 'lat', 'lon'), {'time': np.arange(ns), 'lat': lat, 'lon': lon}, 'q')
    lab = xa.DataArray(ctr, ('time', 'contour'), {'time': np.arange(ns), 'contour': np.arange(23)}, 'ctr')
    cm_r = xa.Contour2D(tr, np.ones(ny), {'X': 'lon', 'Y': 'lat'}, {'Y': 'lat'}, dtype=np.float64, resident=True)
    cm_h = xa.Contour2D(tr, np.ones(ny), {'X': 'lon', 'Y': 'lat'}, {'Y': 'lat'}, dtype=np.float64)
    r1 = cm_r.cal_contour_lengths(lab, latlon=True, periodic=True).values
    r2 = cm_r.cal_contour_lengths(lab, latlon=True, periodic=360).values
    h = cm_h.cal_contour_lengths(lab, latlon=True, periodic=True).values
    assert bits_equal(r1, r2) and bits_equal(r1, h) and bits_equal(h, a[0])
    lk = dict(stride={'lat': 5, 'lon': 4}, min_periods=100, latlon=True, return_levels=True, periodic=True)
    win = {'lat': 15, 'lon': 21}
    r1, l1 = cm_r.cal_local_contour_lengths(win, **lk)
    r2, l2 = cm_r.cal_local_contour_lengths(win, **lk)
    h, lh = cm_h.cal_local_contour_lengths(win, **lk)
    assert bits_equal(r1.values, r2.values) and bits_equal(r1.values, h.values) and bits_equal(h.values, b[0])
    assert bits_equal(l1.values, lh.values) and bits_equal(lh.values, b[1]) and bits_equal(l1.values, l2.values)
    cm_r.close()


def test_bad_periods_rejected(ctx):
    q = np.zeros((1, 5, 6))
    y, x = np.arange(5.0), np.arange(6.0)
    for bad in (0.0, np.nan, np.inf, -6.0, 5.0, 4.0):
        with pytest.raises(nat.XContourHipError) as e:
            ctx.contour_lengths(q, [0.5], y, x, period=bad)
        assert e.value.code == nat.XC_EBADARG and 'period' in str(e.value)
        with pytest.raises(nat.XContourHipError) as e:
            ctx.local_contour_lengths(q, y, x, (3, 3), (1, 1), 1, period=bad)
        assert e.value.code == nat.XC_EBADARG and 'period' in str(e.value)
        lv = np.array([0.5])
        with pytest.raises(nat.XContourHipError) as e:                          # the C host forms check on their own
            _raw_k10(ctx, 'xc_contour_lengths_periodic', q, lv, y, x, 0.0, bad)
        assert e.value.code == nat.XC_EBADARG and 'period' in str(e.value)
        with pytest.raises(nat.XContourHipError) as e:
            _raw_k11(ctx, 'xc_local_contour_lengths_periodic', q, y, x, 0.0, (3, 3), (1, 1), 1, bad)
        assert e.value.code == nat.XC_EBADARG and 'period' in str(e.value)
    with pytest.raises(nat.XContourHipError) as e:
        _raw_k11(ctx, 'xc_local_contour_lengths_periodic', q, y, x, 0.0, (3, 7), (1, 1), 1, 6.0)
    assert e.value.code == nat.XC_EBADARG and 'wider than the ring' in str(e.value)
    with pytest.raises(nat.XContourHipError) as e:                              # a ring of one column
        ctx.contour_lengths(np.zeros((1, 5, 1)), [0.5], y, np.zeros(1), period=1.0)
    assert e.value.code == nat.XC_EBADARG
    assert ctx.last_clen_geometry()['N'] == 0                                   # a failed call leaves the record cleared


# ================================================================== the facade
@pytest.mark.parametrize('transposed', [False, True])
def test_facade_on_the_barotropic_field(baro, transposed):
    q, lat, lon = baro
    c = {'latitude': lat, 'longitude': lon}
    if transposed:
        tr = xa.DataArray(np.ascontiguousarray(q.T), ('longitude', 'latitude'), c, 'absolute_vorticity')
    else:
        tr = xa.DataArray(q, ('latitude', 'longitude'), c, 'absolute_vorticity')
    cm = xa.Contour2D(tr, np.ones(lat.size), {'X': 'longitude', 'Y': 'latitude'}, {'Y': 'latitude'}, dtype=np.float64)
    y, x = CR.plane_coords(lat, lon, True)
    period = float(np.float64(np.deg2rad(np.float32(360.0))))                   # the facade's cast rule
    q64 = q.astype(np.float64)
    ny, nx = q.shape
    ctr = cm.cal_contours(41)
    got = cm.cal_contour_lengths(41, latlon=True, periodic=True)
    assert got.dims == ('contour',) and got.values.shape == (41,)
    assert cm.ctx.last_clen_geometry()['ntile'] == -(-(ny - 1) // 32) * -(-nx // 252)          # nx cell columns
    rt, rn = PR.contour_lengths_fast(q64, ctr.values.astype(np.float64), y, x, period, True)
    ok = ~np.isnan(rt)
    assert ok.sum() > 30 and np.array_equal(np.isnan(got.values), ~ok)
    assert np.max(np.abs(got.values[ok] - rt[ok]) / rt[ok]) <= 1e-12
    plain = cm.cal_contour_lengths(41, latlon=True).values
    assert cm.ctx.last_clen_geometry()['ntile'] == -(-(ny - 1) // 32) * -(-(nx - 1) // 252)
    p0 = np.nan_to_num(plain[ok])
    assert (got.values[ok] >= p0).all() and (got.values[ok] > p0).sum() > 20                    # closed on the sphere: longer

    out, lv = cm.cal_local_contour_lengths(21, stride=5, latlon=True, periodic=True, return_levels=True)
    nwy, nwx = -(-ny // 5), -(-nx // 5)
    assert out.dims == ('latitude', 'longitude') and out.values.shape == (nwy, nwx)
    assert np.array_equal(out.coords['longitude'], lon[::5]) and np.array_equal(out.coords['latitude'], lat[::5])
    # full windows only (min_periods = 21 x 21): the Y edges miss it, the seam columns no longer do
    assert np.isnan(lv.values[:2]).all() and np.isnan(lv.values[-2:]).all() and not np.isnan(lv.values[2:-2]).any()
    rng = np.random.default_rng(3)
    sample = {(int(a), b) for b in (0, 1, 2, nwx - 3, nwx - 2, nwx - 1) for a in rng.integers(2, nwy - 2, 8)}      # the seam stripe
    sample |= {(int(a), int(b)) for a, b in zip(rng.integers(0, nwy, 40), rng.integers(0, nwx, 40))}
    sample = sorted(sample)
    jj, ii = np.array([s[0] for s in sample]), np.array([s[1] for s in sample])
    assert bits_equal(lv.values, PR.window_levels(q64, (21, 21), (5, 5), period))
    rt, rn = PR.local_contour_lengths(q64, lv.values, y, x, period, (21, 21), (5, 5), True, sample=sample)
    check(out.values[jj, ii], rn[jj, ii], rt[jj, ii], rn[jj, ii], 'local, transposed=%s' % transposed)
    assert (rn[jj, ii] > 0).sum() > 40
    with pytest.raises(Exception, match='window should not be wider than the periodic dim longitude'):
        cm.cal_local_contour_lengths({'latitude': 5, 'longitude': nx + 1}, latlon=True, periodic=True)
