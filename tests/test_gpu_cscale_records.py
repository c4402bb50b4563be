"""xc_coarsen / xc_contour_lengths_scales (K26), the C entries in host and device form.  The coarse plane against cscale_ref.coarsen,
every element BIT FOR BIT (additions and one division, the same in numpy and on the device: no tolerance); the lengths of every
ratio bit for bit, the segment counts exactly, what xc_contour_lengths / _periodic returns for the restatement's coarse plane and
coordinates.  test_cscale_host.py shows on the CPU that a wrong rule disagrees with the restatement on these inputs.  Every output
is followed by guard elements, and a refused call leaves outputs filled with a pattern as they were."""
import ctypes as C

import numpy as np
import pytest

import cscale_ref as R
from gpu_common import same_bits
from xcontour_amd import _native as nat

pytestmark = pytest.mark.gpu

GUARD = 8
PAT = -1.2345e30
UPAT = np.uint64(0xABCDABCDABCDABCD)
F32, F64 = np.float32, np.float64


def _err(ctx):
    return ctx.lib.xc_last_error(ctx.handle).decode()


def coarsen_host(ctx, q, r, skipna=False):
    q = np.ascontiguousarray(q)
    S, ny, nx = q.shape
    n = S * (ny // max(r, 1)) * (nx // max(r, 1)) if r > 0 else 0
    out = np.full(n + GUARD, PAT)
    rc = ctx.lib.xc_coarsen(ctx.handle, q.ctypes.data, nat.dtype_code(q.dtype), S, ny, nx, r, int(skipna), out.ctypes.data)
    assert (out[n:] == PAT).all(), 'a guard element was written'
    return rc, out[:n]


def coarsen_dev(ctx, q, r, skipna=False, shift=0):
    """through xc_coarsen_dev; shift: the tracer starts `shift` elements into its allocation"""
    q = np.ascontiguousarray(q)
    S, ny, nx = q.shape
    n = S * (ny // max(r, 1)) * (nx // max(r, 1)) if r > 0 else 0
    qpad = np.concatenate((np.zeros(shift, dtype=q.dtype), q.ravel()))
    with ctx._temporaries([qpad, np.full(n + GUARD, PAT)], []) as (dq, do):
        rc = ctx.lib.xc_coarsen_dev(ctx.handle, dq.ptr + shift * q.dtype.itemsize, nat.dtype_code(q.dtype), S, ny, nx, r, int(skipna), do.ptr)
        ctx.sync()
        out = do.download((n + GUARD,), F64)
    assert (out[n:] == PAT).all(), 'a guard element was written'
    return rc, out[:n]


def check_coarsen(ctx, q, r, skipna, what=''):
    ref = R.coarsen(q, r, skipna)
    for name, call, kw in (('host', coarsen_host, {}), ('dev', coarsen_dev, {}), ('dev shifted', coarsen_dev, {'shift': 3})):
        rc, got = call(ctx, q, r, skipna, **kw)
        assert rc == 0, '%s %s: status %d (%s)' % (what, name, rc, _err(ctx))
        same_bits(got.reshape(ref.shape), ref, '%s %s ratio %d skipna %d' % (what, name, r, skipna))
    return ctx.last_cscale_geometry()


@pytest.mark.parametrize('skipna', [False, True], ids=['nan', 'skipna'])
@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
@pytest.mark.parametrize('shape', [(1, 13, 37), (2, 70, 530)], ids=lambda s: '%dx%dx%d' % s)
def test_coarsen_planes_with_tails(ctx, shape, dtype, skipna):
    """both shapes leave tails in both directions; NaN at a block's first, last and only finite node, an all-NaN block row and
    block, +-inf (cscale_ref.with_specials).  13 // 5 = 13 // 6 = 2: exactly two coarse rows; 70 // 64 = 1"""
    S, ny, nx = shape
    for r in (1, 2, 3, 5, 6, 8, 64):
        if ny // r < 1 or nx // r < 1:
            continue
        q = R.with_specials(R.field(S, ny, nx, dtype, seed=r), r)
        g = check_coarsen(ctx, q, r, skipna, '%r %s' % (shape, np.dtype(dtype).name))
        ty, tx = g['tile'][0]
        assert g['ratio'] == [r] and g['q_dtype'] == np.dtype(dtype) and g['block'] == 256
        assert g['grid'][0] == (-(-(nx // r) // tx), -(-(ny // r) // ty), S)


@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
@pytest.mark.parametrize('r', [2, 3, 8, 17, 33])
def test_coarsen_across_tile_edges(ctx, r, dtype):
    """a plane the launch record shows to take two tiles in x and two in y, the last of each partial: the tile of this ratio is
    read from the record of a small call, then the plane is built to one full tile plus a part of one (half a tile where that
    stays under 600 columns, else one column), with a trimmed tail"""
    rc, _ = coarsen_host(ctx, np.zeros((1, 2 * r, 2 * r), dtype=dtype), r)
    assert rc == 0
    ty, tx = ctx.last_cscale_geometry()['tile'][0]
    cny = ty + 1
    cnx = tx + tx // 2 if (tx + tx // 2) * r < 600 else tx + 1
    ny, nx = cny * r + r - 1, cnx * r + 1
    assert ny < 300 and nx < 600
    q = R.with_specials(R.field(2, ny, nx, dtype, seed=r), r)
    for skipna in (False, True):
        g = check_coarsen(ctx, q, r, skipna, 'tiles')
        assert g['grid'][0] == (2, 2, 2) and cnx % tx and cny % ty


# ---------------------------------------------------------------------------------------------------- lengths per ratio
def scales(ctx, q, y, x, lev, ratios, period=0.0, radius=0.0, skipna=False, nseg=True, dev=False, nratio=None):
    """one xc_contour_lengths_scales(_dev) call -> (rc, lengths (nratio, S, N), counts or None)"""
    q, lev = np.ascontiguousarray(q), np.ascontiguousarray(lev, dtype=F64)
    y, x = np.ascontiguousarray(y, dtype=F64), np.ascontiguousarray(x, dtype=F64)
    S, ny, nx = q.shape
    N, nr = lev.shape[-1], len(ratios)
    n = nr * S * N
    rr = (C.c_int * max(nr, 1))(*ratios)
    nr = nr if nratio is None else nratio
    lens, cnts = np.full(n + GUARD, PAT), np.full(n + GUARD, UPAT, dtype=np.uint64)
    args = (nat.dtype_code(q.dtype), S, ny, nx)
    tail = (float(period), float(radius), rr, nr, int(skipna))
    if dev:
        with ctx._temporaries([q, y, x, lev, lens, cnts], []) as (dq, dy, dx, dc, dl, dn):
            rc = ctx.lib.xc_contour_lengths_scales_dev(ctx.handle, dq.ptr, *args, dy.ptr, dx.ptr, *tail, dc.ptr, N, int(lev.ndim == 2),
                                                       dl.ptr, dn.ptr if nseg else None)
            ctx.sync()
            lens, cnts = dl.download(lens.shape, F64), dn.download(cnts.shape, np.uint64)
    else:
        rc = ctx.lib.xc_contour_lengths_scales(ctx.handle, q.ctypes.data, *args, y.ctypes.data, x.ctypes.data, *tail, lev.ctypes.data, N,
                                               int(lev.ndim == 2), lens.ctypes.data, cnts.ctypes.data if nseg else None)
    assert (lens[n:] == PAT).all() and (cnts[n:] == UPAT).all(), 'a guard element was written'
    if not nseg:
        assert (cnts == UPAT).all()
    shape = (len(ratios), S, N)
    return rc, lens[:n].reshape(shape), cnts[:n].reshape(shape) if nseg else None


def plane_inputs(dtype, radius, S=2, ny=48, nx=96, N=7):
    q = R.field(S, ny, nx, dtype, seed=11)
    if radius > 0:
        y = np.deg2rad(np.linspace(-80, 80, ny).astype(F32)).astype(F64)
        x = np.deg2rad((np.arange(nx) * (360.0 / nx)).astype(F32)).astype(F64)
        period = float(np.deg2rad(F32(360.0)))
    else:
        y, x = R.coords(ny, 1), R.coords(nx, 2)
        period = float(x[-1] - x[0] + 1.5)
    lev = np.stack([R.levels(R.coarsen(q[s], 4), N) * (1.0 + 0.01 * s) for s in range(S)])
    return q, y, x, period, lev


@pytest.mark.parametrize('dev', [False, True], ids=['host', 'dev'])
@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
@pytest.mark.parametrize('radius', [0.0, 6371200.0], ids=['plane', 'sphere'])
@pytest.mark.parametrize('periodic', [False, True], ids=['plain', 'periodic'])
def test_lengths_per_ratio_are_k10_on_the_restated_plane(ctx, periodic, radius, dtype, dev):
    """two slabs, levels per slab, ratios out of order and with a repeat; every row against the K10 entry on the restatement's
    coarse plane and coordinates; the ratio-1 row against K10 on the input itself"""
    q, y, x, period, lev = plane_inputs(dtype, radius)
    ratios = [4, 1, 2, 8, 2, 3]
    rc, lens, cnts = scales(ctx, q, y, x, lev, ratios, period if periodic else 0.0, radius, dev=dev)
    assert rc == 0, _err(ctx)
    g = ctx.last_cscale_geometry()
    assert g['ratio'] == ratios and g['grid'][1] == (0, 0, 0) and g['grid'][0][2] == 2
    crossed = 0
    for k, r in enumerate(ratios):
        plane = q if r == 1 else R.coarsen(q, r)
        rl, rn = ctx.contour_lengths(plane, lev, R.coarsen_coords(y, r), R.coarsen_coords(x, r), radius=radius, period=period if periodic else None)
        same_bits(lens[k], rl, 'ratio %d lengths' % r)
        assert np.array_equal(cnts[k], rn), 'ratio %d counts' % r
        crossed += int((rn > 0).sum())
        if r == 1:
            assert (rn > 0).all()                                    # the levels lie inside the field: nothing here is all NaN
    assert crossed > lev.size                                        # ... and the coarse planes are crossed too
    same_bits(lens[2], lens[4], 'the repeated ratio')
    rc, lens2, none = scales(ctx, q, y, x, lev, ratios, period if periodic else 0.0, radius, dev=dev, nseg=False)
    assert rc == 0 and none is None
    same_bits(lens2, lens, 'without out_nseg')


def test_lengths_skipna_and_shared_levels(ctx):
    q, y, x, period, lev = plane_inputs(F64, 0.0)
    q = R.with_specials(q, 4)
    for skipna in (False, True):
        rc, lens, cnts = scales(ctx, q, y, x, lev[0], [4, 2], 0.0, 0.0, skipna=skipna)
        assert rc == 0, _err(ctx)
        for k, r in enumerate((4, 2)):
            rl, rn = ctx.contour_lengths(R.coarsen(q, r, skipna), lev[0], R.coarsen_coords(y, r), R.coarsen_coords(x, r))
            same_bits(lens[k], rl, 'skipna %d ratio %d' % (skipna, r))
            assert np.array_equal(cnts[k], rn)


# ---------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize('dev', [False, True], ids=['host', 'dev'])
def test_refusals_write_nothing(ctx, dev):
    q, y, x, period, lev = plane_inputs(F64, 0.0, ny=12, nx=16)
    for ratios, per, nratio, text in (([2, 0], 0.0, None, 'ratio 0'), ([65], 0.0, None, 'ratio 65'), ([2], 0.0, 0, 'nratio'),
                                      ([1] * 9, 0.0, None, 'nratio'), ([2, 3], period, None, 'ratio 3'),     # 16 % 3 != 0 on a ring
                                      ([2, 7], 0.0, None, 'ratio 7')):                                    # one coarse row
        rc, lens, cnts = scales(ctx, q, y, x, lev, ratios, per, dev=dev, nratio=nratio)
        assert rc == nat.XC_EBADARG and text in _err(ctx), (ratios, _err(ctx))
        assert (lens == PAT).all() and (cnts == UPAT).all()
        g = ctx.last_cscale_geometry()
        assert g['q_dtype'] is None and g['ratio'] == []
    rc, lens, _ = scales(ctx, q[:, :, :6], y, x[:6], lev, [4], 0.0, dev=dev)        # three coarse rows, but one coarse column
    assert rc == nat.XC_EBADARG and 'ratio 4' in _err(ctx) and (lens == PAT).all()
    assert R.refusal(12, 16, [7]) == R.refusal(12, 6, [4]) == R.refusal(12, 16, [3], periodic=True) == R.XC_EBADARG
    rc, lens, _ = scales(ctx, q, y, x, lev, [6], 0.0, dev=dev)      # two coarse rows, two coarse columns: the smallest plane taken
    assert rc == 0, _err(ctx)
    rc, lens, _ = scales(ctx, q, y, x, lev, [4], period, dev=dev)   # ... and a ring
    assert rc == 0, _err(ctx)
    if not dev:                                                      # what the host form can read: levels and coordinates
        rc, lens, cnts = scales(ctx, q, y, x, lev[:, ::-1], [2])
        assert rc == nat.XC_EEDGES and (lens == PAT).all() and (cnts == UPAT).all()
        rc, lens, _ = scales(ctx, q, np.where(y == y[3], np.inf, y), x, lev, [2])
        assert rc == nat.XC_EBADARG and (lens == PAT).all()
        rc, lens, _ = scales(ctx, q, y, x, lev, [2], period=-period)
        assert rc == nat.XC_EBADARG and (lens == PAT).all()


def test_coarsen_refusals(ctx):
    q = R.field(1, 12, 16)
    for call in (coarsen_host, coarsen_dev):
        for r in (0, 65, 13, 17):
            rc, out = call(ctx, q, r)
            assert rc == nat.XC_EBADARG and 'ratio %d' % r in _err(ctx)
            assert ctx.last_cscale_geometry()['ratio'] == []
