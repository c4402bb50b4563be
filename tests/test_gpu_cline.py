"""K15 (xc_contour_line_integrals, Context.contour_line_integrals) on the GPU against the numpy restatement cline_ref: segment
counts and the NaN pattern exact, lengths within 1e-12 relative (K10's bar), integrals within 1e-12 of the sum of |term| (the
same bar on the absolute sum: signed terms cancel).  Shapes sit on the tile walk's boundaries: tiles are 32 x 252 cells, waves 63
cells."""
import numpy as np
import pytest

import clength_ref as CR
import clength_periodic_ref as PR
import cline_ref as LR
from gpu_common import same_bits

pytestmark = pytest.mark.gpu

NY, NX = 35, 256                                             # 2 x 2 tiles
PERIOD_LL = float(np.float64(np.deg2rad(np.float32(360.0))))


def check(got, ref, what=''):
    integ, length, nseg = (np.asarray(v) for v in got)
    r_int, r_len, r_n, r_scale = ref
    assert np.array_equal(nseg.astype(np.int64), r_n), what
    assert np.array_equal(np.isnan(length), np.isnan(r_len)), what
    assert np.array_equal(np.isnan(integ), np.isnan(r_int)), what
    ok = ~np.isnan(r_len)
    if ok.any():
        e = np.abs(length[ok] - r_len[ok]) / np.abs(r_len[ok])
        assert e.max() <= 1e-12, '%s: length rel %.3g' % (what, e.max())
    ok = ~np.isnan(r_int)
    if ok.any():
        e = np.abs(integ[ok] - r_int[ok]) / r_scale[ok]
        print('%s: integral error / sum |term| = %.3g' % (what, np.nanmax(e)))
        assert np.all(np.abs(integ[ok] - r_int[ok]) <= 1e-12 * r_scale[ok]), '%s: integral %.3g of sum |term|' % (what, np.nanmax(e))


def coords(ny, nx, latlon):
    if latlon:
        return CR.plane_coords(np.linspace(-80.0, 80.0, ny), np.linspace(0.0, 360.0, nx, endpoint=False), True)
    return CR.hashed_coords(ny, 3, scale=700.0), CR.hashed_coords(nx, 5, scale=1100.0)


def period_of(x, latlon):
    return PERIOD_LL if latlon else float(x[-1] - x[0] + 1300.0)


def radius(latlon):
    return CR.RADIUS if latlon else 0.0


def f64(a):
    return np.asarray(a, dtype=np.float64)


@pytest.mark.parametrize('latlon', [False, True])
@pytest.mark.parametrize('tf', [np.float32, np.float64])
@pytest.mark.parametrize('tq', [np.float32, np.float64])
def test_every_dtype_pair_on_two_by_two_tiles(ctx, tq, tf, latlon):
    rng = np.random.default_rng(21)
    q = rng.standard_normal((1, NY, NX)).astype(tq)
    F = (3.0 * rng.standard_normal((1, NY, NX)) + 1.0).astype(tf)
    y, x = coords(NY, NX, latlon)
    lv = np.linspace(-2.0, 2.0, 37)
    got = ctx.contour_line_integrals(q, F, lv, y, x, radius=radius(latlon))
    g = ctx.last_clen_geometry()
    assert g['ntile'] == 4 and g['ngroup'] == 1 and g['q_dtype'] == np.dtype(tq)
    check(got, LR.stack(f64(q), f64(F), lv, y, x, latlon), 'q %s F %s latlon %s' % (tq.__name__, tf.__name__, latlon))


def test_level_groups(ctx):
    rng = np.random.default_rng(22)
    q = rng.standard_normal((1, NY, NX))
    F = rng.standard_normal((1, NY, NX))
    y, x = coords(NY, NX, False)
    lv = np.sort(rng.uniform(-3.0, 3.0, 600))
    got = ctx.contour_line_integrals(q, F, lv, y, x)
    g = ctx.last_clen_geometry()
    assert g['ngroup'] >= 2 and g['ntile'] == 4 and g['N'] == 600 and g['ncopy'] == 1
    check(got, LR.stack(q, F, lv, y, x), '600 levels')


@pytest.mark.parametrize('latlon', [False, True])
@pytest.mark.parametrize('nx,ntile', [(252, 2), (253, 4), (2, 2)])
def test_periodic_seam(ctx, nx, ntile, latlon):
    """nx = 252: the seam cell's right neighbour is the wave's halo lane; 253: the seam cell is alone in a second tile column; 2: the
    ring of two cells.  The periodic call against the restatement, and bit for bit the plain call on the extended plane"""
    rng = np.random.default_rng(23 + nx)
    q = rng.standard_normal((2, NY, nx))
    F = rng.standard_normal((2, NY, nx)) - 0.5
    y, x = coords(NY, nx, latlon)
    P = period_of(x, latlon)
    lv = np.linspace(-1.5, 1.5, 19)
    got = ctx.contour_line_integrals(q, F, lv, y, x, radius=radius(latlon), period=P)
    assert ctx.last_clen_geometry()['ntile'] == ntile
    check(got, LR.stack(q, F, lv, y, x, latlon, period=P), 'ring nx %d' % nx)
    qe, xe = PR.extend_plane(q, x, P)
    Fe, _ = PR.extend_plane(F, x, P)
    ext = ctx.contour_line_integrals(np.ascontiguousarray(qe), np.ascontiguousarray(Fe), lv, y, xe, radius=radius(latlon))
    same_bits(got[0], ext[0], 'integral'); same_bits(got[1], ext[1], 'length')
    assert np.array_equal(got[2], ext[2])
    # and the seam is really traced: more segments than without the period
    assert got[2].sum() > ctx.contour_line_integrals(q, F, lv, y, x, radius=radius(latlon))[2].sum()


def fields(kind, rng, ns, ny, nx):
    """-> (q, F, levels)"""
    F = 2.0 * rng.standard_normal((ns, ny, nx)) + 0.5
    lv = np.linspace(-2.0, 2.0, 29)
    if kind == 'saddle':                                     # the checkerboard of the K10 tests
        q = np.indices((ny, nx)).sum(0) % 2 * 2.0 - 1.0 + 0.3 * rng.standard_normal((ns, ny, nx))
    elif kind == 'integer':                                  # levels exactly on node values
        q = rng.integers(0, 6, size=(ns, ny, nx)).astype(np.float64)
        lv = np.array([-1.0, 0.0, 1.0, 2.0, 2.5, 3.0, 4.0, 5.0, 6.0])
    else:
        q = rng.standard_normal((ns, ny, nx))
    if kind == 'nan_q':
        q[rng.random(q.shape) < 0.03] = np.nan
    if kind == 'nan_f':
        F[rng.random(F.shape) < 0.03] = np.nan
    if kind == 'inf_f':
        F[0, ny // 2, nx // 2] = np.inf
    return q, F, lv


@pytest.mark.parametrize('kind', ['saddle', 'integer', 'nan_q', 'nan_f', 'inf_f'])
def test_fields(ctx, kind):
    rng = np.random.default_rng(31)
    q, F, lv = fields(kind, rng, 2, NY, NX)
    for latlon in (False, True):
        y, x = coords(NY, NX, latlon)
        ref = LR.stack(q, F, lv, y, x, latlon)
        got = ctx.contour_line_integrals(q, F, lv, y, x, radius=radius(latlon))
        check(got, ref, '%s latlon %s' % (kind, latlon))
        klen, kn = ctx.contour_lengths(q, lv, y, x, radius=radius(latlon))
        if kind in ('nan_f', 'inf_f'):                       # segments are skipped, and not counted (an infinite FIRST node of an edge
            assert (got[2] <= kn).all() and got[2].sum() < kn.sum()      # gives a NaN end-point value, (F1 - inf) t + inf)
        else:                                                # the length channel is K10's, bit for bit
            same_bits(got[1], klen, kind + ' length'); assert np.array_equal(got[2], kn)
        if kind == 'inf_f':                                  # some level of slab 0 met the infinite node: its integral alone is NaN
            hit = np.isnan(ref[0][0]) & ~np.isnan(ref[1][0])
            assert hit.any() and not (np.isnan(ref[0][1]) & ~np.isnan(ref[1][1])).any()
            assert np.array_equal(np.isnan(got[0][0]) & ~np.isnan(got[1][0]), hit)


@pytest.mark.parametrize('periodic', [False, True])
def test_length_channel_is_k10(ctx, periodic):
    rng = np.random.default_rng(41)
    q = rng.standard_normal((2, NY, NX)).astype(np.float32)
    F = rng.standard_normal((2, NY, NX))
    lv = np.linspace(-2.5, 2.5, 41)
    for latlon in (False, True):
        y, x = coords(NY, NX, latlon)
        P = period_of(x, latlon) if periodic else None
        got = ctx.contour_line_integrals(q, F, lv, y, x, radius=radius(latlon), period=P)
        klen, kn = ctx.contour_lengths(q, lv, y, x, radius=radius(latlon), period=P)
        same_bits(got[1], klen, 'length'); assert np.array_equal(got[2], kn)


def test_constant_integrand_is_the_length_bit_for_bit(ctx):
    """F = 1: every term equals its length exactly, both channels sum the same integer chunks (each on its own window, 180 bits
    deep), so the integral is the length, bit for bit"""
    ya, xa_ = np.meshgrid(np.linspace(-1.4, 1.4, NY), np.linspace(0.0, 6.2, NX), indexing='ij')
    q = (np.sin(ya) * 2.0 + 0.3 * np.cos(3 * xa_) * np.cos(ya) ** 2 + 0.1 * np.sin(5 * xa_ + 2 * ya))[None]
    y, x = coords(NY, NX, False)
    lv = np.linspace(q.min(), q.max(), 39)[1:-1]
    for F in (np.ones_like(q), np.ones(q.shape, dtype=np.float32)):
        integ, length, nseg = ctx.contour_line_integrals(q, F, lv, y, x)
        assert (nseg > 0).all()
        same_bits(integ, length, 'F = 1')


def test_reproducible_alone_and_in_a_stack(ctx):
    rng = np.random.default_rng(51)
    q = rng.standard_normal((3, NY, NX))
    F = rng.standard_normal((3, NY, NX)) * np.array([1.0, 1e-6, 1e9])[:, None, None]      # a window of its own per slab
    lv = np.sort(rng.uniform(-2.0, 2.0, (3, 23)), axis=1)                                   # per-slab levels
    y, x = coords(NY, NX, True)
    a = ctx.contour_line_integrals(q, F, lv, y, x, radius=CR.RADIUS)
    b = ctx.contour_line_integrals(q, F, lv, y, x, radius=CR.RADIUS)
    check(a, LR.stack(q, F, lv, y, x, True), '3 slabs')
    for u, v in zip(a, b):
        same_bits(u, v, 'repeat')
    for s in range(3):
        one = ctx.contour_line_integrals(q[s:s + 1], F[s:s + 1], lv[s], y, x, radius=CR.RADIUS)
        for u, v in zip(one, a):
            same_bits(u[0], v[s], 'slab %d alone' % s)


def test_bad_input_rejected(ctx):
    from xcontour_amd import _native as nat
    q = np.zeros((1, 5, 6))
    y, x = np.arange(5.0), np.arange(6.0)
    with pytest.raises(nat.XContourHipError) as e:
        ctx.contour_line_integrals(q, np.zeros((1, 5, 5)), [0.5], y, x)
    assert e.value.code == nat.XC_EBADARG
    with pytest.raises(nat.XContourHipError) as e:
        ctx.contour_line_integrals(q, q, [1.0, 0.5], y, x)
    assert e.value.code == nat.XC_EEDGES
    with pytest.raises(nat.XContourHipError) as e:
        ctx.contour_line_integrals(q, q, [0.5], y, x, period=3.0)
    assert e.value.code == nat.XC_EBADARG
    assert ctx.last_clen_geometry()['q_dtype'] is None
