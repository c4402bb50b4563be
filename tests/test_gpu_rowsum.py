"""xc_rowsum (K2 k_rowsum: one wave a row, four rows a block) on weights and masks whose every partial sum is exact -- small integers
times a power of two -- so that any order of addition gives the same double and the reference is math.fsum per row, BIT FOR BIT.
Every mask dtype, weight rank and both `multiply` settings, rows on both sides of a block of four, columns on both sides of a wave
of 64, the mask values that tell `mask * dA` from `where(mask == 1)`, and the refusals of launch_rowsum."""
import math

import numpy as np
import pytest

from gpu_common import same_bits
from xcontour_amd import _native as nat

pytestmark = pytest.mark.gpu

NYS = (1, 3, 4, 5, 9)
NXS = (1, 63, 64, 65, 129, 300)
SHAPES = [(ny, nx) for ny in NYS for nx in NXS]


def scaled(rng, shape):
    """integers in [-512, 512] times 2^-6: 300 of them, times a mask of 2 or -1 or 1 - 2^-24, sum exactly in a double in any order"""
    return rng.integers(-512, 513, size=shape).astype(np.float64) * 2.0 ** -6


def mask_of(rng, kind, shape, multiply):
    """None, or a float32 / float64 mask of 1, 0, 2, -1, the number just below 1 and NaN.  (The float64 number just below 1 times a
    weight is not exact in a sum of 300: under `multiply` only the float32 mask holds it; without `multiply` it must simply not count.)"""
    if kind is None:
        return None
    dt = np.dtype(kind).type
    values = [dt(1), dt(0), dt(2), dt(-1), np.nextafter(dt(1), dt(0)), dt(np.nan), dt(1), dt(1)]
    if multiply and dt is np.float64:
        values[4] = dt(1)
    assert values[4] == 1 or (values[4] < 1 and dt(1) - values[4] <= 2.0 ** -24)
    m = np.array(values, dtype=dt)[rng.integers(0, len(values), size=shape)]
    return m


def weights_of(rng, rank, ny, nx, nan=False):
    if rank == nat.XC_DA_NONE:
        return None
    w = scaled(rng, (ny,) if rank == nat.XC_DA_ROW else (ny, nx))
    if nan:
        w[(ny // 2,) if rank == nat.XC_DA_ROW else (ny // 2, nx // 2)] = np.nan
    return w


def reference(mask, w, ny, nx, multiply):
    """per row: (mask * dA) summed without its NaN (multiply), or dA summed where mask == 1 -- math.fsum of the terms"""
    full = np.ones((ny, nx)) if w is None else (np.repeat(w[:, None], nx, axis=1) if w.ndim == 1 else w)
    out = np.empty(ny)
    for y in range(ny):
        if multiply:
            t = full[y] if mask is None else mask[y].astype(np.float64) * full[y]
            t = t[~np.isnan(t)]
        else:
            t = full[y] if mask is None else full[y][mask[y] == 1]
        out[y] = np.nan if np.isnan(t).any() else math.fsum(t.tolist())
    return out


def check(ctx, mask, w, ny, nx, multiply, what):
    got = ctx.rowsum(mask, w, ny, nx, multiply=multiply)
    assert got.shape == (ny,)
    ref = reference(mask, w, ny, nx, multiply)
    same_bits(got + 0.0, ref + 0.0, what)                                     # (+ 0.0: an empty or cancelled sum is a zero of either sign)
    return got


@pytest.mark.parametrize('rank', [nat.XC_DA_NONE, nat.XC_DA_ROW, nat.XC_DA_PLANE], ids=['none', 'row', 'plane'])
@pytest.mark.parametrize('kind', [None, np.float32, np.float64], ids=['nomask', 'mask32', 'mask64'])
def test_rowsum_equals_fsum_at_every_shape(ctx, kind, rank):
    rng = np.random.default_rng(2 + rank)
    for ny, nx in SHAPES:
        for multiply in (False, True):
            mask = mask_of(rng, kind, (ny, nx), multiply)
            w = weights_of(rng, rank, ny, nx)
            check(ctx, mask, w, ny, nx, multiply, '%s rank %d %d x %d multiply %d' % (kind and np.dtype(kind).name, rank, ny, nx, multiply))


@pytest.mark.parametrize('kind', [np.float32, np.float64], ids=['mask32', 'mask64'])
def test_mask_values_one_by_one(ctx, kind):
    """a row per mask value, all of its cells that value: with `multiply` 2 counts twice, -1 negates and a NaN product is skipped;
    without it only exact 1 counts -- not 2, not the number just below 1, not NaN"""
    dt = np.dtype(kind).type
    below = np.nextafter(dt(1), dt(0))
    values = [dt(1), dt(0), dt(2), dt(-1), below, dt(np.nan)]
    for nx in (1, 64, 65, 300):
        ny = len(values)
        mask = np.repeat(np.array(values, dtype=dt)[:, None], nx, axis=1)
        rng = np.random.default_rng(nx)
        w = np.abs(scaled(rng, (ny, nx))) + 1.0
        total = np.array([math.fsum(r.tolist()) for r in w])
        got = check(ctx, mask, w, ny, nx, False, 'where(mask == 1) nx %d' % nx)
        assert got.tolist() == [total[0], 0.0, 0.0, 0.0, 0.0, 0.0]
        w2 = w.copy()
        if dt is np.float64:
            w2[4] = 0.0                                                       # (its product with 1 - 2^-53 is not exact in a sum)
        got = check(ctx, mask, w2, ny, nx, True, 'mask * dA nx %d' % nx)
        assert got[:4].tolist() == [total[0], 0.0, 2 * total[2], -total[3]] and got[5] == 0.0
        if dt is np.float32:
            assert 0 < got[4] < total[4] and got[4] == total[4] - total[4] * 2.0 ** -24


@pytest.mark.parametrize('kind', [None, np.float32, np.float64], ids=['nomask', 'mask32', 'mask64'])
@pytest.mark.parametrize('rank', [nat.XC_DA_ROW, nat.XC_DA_PLANE], ids=['row', 'plane'])
def test_nan_weights(ctx, kind, rank):
    """without `multiply` a NaN weight under a counted cell shows (NaN for that row alone) and one under a cell that is not counted
    does not; with `multiply` the NaN product is skipped"""
    for ny, nx in ((5, 65), (9, 300), (1, 1)):
        rng = np.random.default_rng(ny)
        w = weights_of(rng, rank, ny, nx, nan=True)
        y, x = ny // 2, nx // 2
        for counted in (True, False):
            mask = None
            if kind is not None:
                mask = np.ones((ny, nx), dtype=kind)
                mask[:, ::3] = 0
                mask[y, :] = 1 if counted else 0
                if rank == nat.XC_DA_PLANE and not counted:
                    mask[y, :] = 1
                    mask[y, x] = 2
            got = check(ctx, mask, w, ny, nx, False, 'NaN weight, where(): rank %d %d x %d counted %d' % (rank, ny, nx, counted))
            shows = kind is None or counted
            assert np.isnan(got[y]) == shows and not np.isnan(np.delete(got, y)).any()
            got = check(ctx, mask, w, ny, nx, True, 'NaN weight, multiply: rank %d %d x %d' % (rank, ny, nx))
            assert not np.isnan(got).any()


def test_refusals_leave_the_output_alone(ctx):
    ny, nx = 5, 65
    rng = np.random.default_rng(7)
    mask, w = np.ones((ny, nx), dtype=np.float32), scaled(rng, (ny, nx))
    fill = np.full(ny, -1.2345e300)
    E = nat.XC_EBADARG
    with ctx._temporaries([mask, w, fill], []) as (dm, dw, dout):
        dev = lambda m, mdt, d, rank, ny_, nx_, out: ctx.lib.xc_rowsum_dev(ctx.handle, m, mdt, d, rank, ny_, nx_, 0, out)
        for rank in (nat.XC_DA_SLAB, 7, -1):
            assert dev(dm.ptr, nat.XC_F32, dw.ptr, rank, ny, nx, dout.ptr) == E, 'rank %d' % rank
        for rank in (nat.XC_DA_ROW, nat.XC_DA_PLANE):
            assert dev(dm.ptr, nat.XC_F32, None, rank, ny, nx, dout.ptr) == E, 'NULL weights with rank %d' % rank
        for mdt in (2, -1):
            assert dev(dm.ptr, mdt, dw.ptr, nat.XC_DA_PLANE, ny, nx, dout.ptr) == E, 'mask dtype %d' % mdt
        assert dev(dm.ptr, nat.XC_F32, dw.ptr, nat.XC_DA_PLANE, 0, nx, dout.ptr) == E
        assert dev(dm.ptr, nat.XC_F32, dw.ptr, nat.XC_DA_PLANE, ny, 0, dout.ptr) == E
        assert dev(dm.ptr, nat.XC_F32, dw.ptr, nat.XC_DA_PLANE, ny, nx, None) == E
        assert b'rowsum' in ctx.lib.xc_last_error(ctx.handle)
        assert dout.download((ny,), np.float64).tobytes() == fill.tobytes(), 'a refused call wrote'
        # ... and the same call with nothing wrong, and with no mask (then the mask dtype is not looked at)
        assert dev(dm.ptr, nat.XC_F32, dw.ptr, nat.XC_DA_PLANE, ny, nx, dout.ptr) == 0
        same_bits(dout.download((ny,), np.float64), reference(mask, w, ny, nx, False), 'the device form')
        assert dev(None, 9, dw.ptr, nat.XC_DA_PLANE, ny, nx, dout.ptr) == 0
        same_bits(dout.download((ny,), np.float64), reference(None, w, ny, nx, False), 'the device form without a mask')
    out = np.empty(ny)
    host = lambda m, mdt, d, rank: ctx.lib.xc_rowsum(ctx.handle, nat._ptr(m), mdt, nat._ptr(d), rank, ny, nx, 0, nat._ptr(out))
    assert host(mask, 2, w, nat.XC_DA_PLANE) == E and host(mask, nat.XC_F32, None, nat.XC_DA_ROW) == E
    assert host(mask, nat.XC_F32, w, nat.XC_DA_SLAB) == E and host(mask, nat.XC_F32, w, 7) == E
