"""xc_contour_map / xc_contour_map_dev (K25), the C entries, against cmap_ref.contour_map: every element BIT FOR BIT (numpy's arr_interp
and the device's interp_eval are the same arithmetic: no tolerance).  The inputs are cmap_ref's; test_cmap_host.py shows on the CPU
that a wrong rule disagrees with the restatement on them.  Every output plane is followed by guard elements, and a refused call
leaves planes filled with a pattern as they were."""
import ctypes as C

import numpy as np
import pytest

import cmap_ref as R
from gpu_common import same_bits
from xcontour_amd import _native as nat

pytestmark = pytest.mark.gpu

GUARD = 8
PAT = -1.2345e30
F32, F64 = np.float32, np.float64
TILE = nat.XC_CMAP_TILE


def _flags(arrs):
    return (C.c_int * max(len(arrs), 1))(*[1 if np.ndim(a) == 2 else 0 for a in arrs])


def host_call(ctx, q, xp, fps, out_dtype=F64, N=None, nv=None, q_code=None, out_code=None, nslab=None):
    """one xc_contour_map call -> (rc, planes); the keyword overrides hand the entry what the arrays would not"""
    q, xp = np.ascontiguousarray(q), np.ascontiguousarray(xp, dtype=F64)
    fps = [np.ascontiguousarray(f, dtype=F64) for f in fps]
    S, ny, nx = q.shape
    outs = [np.full(S * ny * nx + GUARD, PAT, dtype=out_dtype) for _ in range(max(len(fps), 1))]
    n = len(fps) if nv is None else nv
    fp = (C.c_void_p * max(len(fps), 1))(*[f.ctypes.data for f in fps])
    op = (C.c_void_p * len(outs))(*[o.ctypes.data for o in outs])
    rc = ctx.lib.xc_contour_map(ctx.handle, q.ctypes.data, nat.dtype_code(q.dtype) if q_code is None else q_code, S if nslab is None else nslab,
                                ny, nx, xp.ctypes.data, xp.shape[-1] if N is None else N, 1 if xp.ndim == 2 else 0, n, fp, _flags(fps), op,
                                nat.dtype_code(np.dtype(out_dtype)) if out_code is None else out_code)
    for o in outs:
        assert (o[S * ny * nx:] == out_dtype(PAT)).all(), 'a guard element was written'
    return rc, [o[:S * ny * nx].reshape(S, ny, nx) for o in outs]


def dev_call(ctx, q, xp, fps, out_dtype=F64, N=None, nv=None, nslab=None, shift=0):
    """the same through xc_contour_map_dev; shift: the tracer and the planes start `shift` elements into their allocations"""
    q, xp = np.ascontiguousarray(q), np.ascontiguousarray(xp, dtype=F64)
    fps = [np.ascontiguousarray(f, dtype=F64) for f in fps]
    S, ny, nx = q.shape
    cells = S * ny * nx
    fresh = [np.full(shift + cells + GUARD, PAT, dtype=out_dtype) for _ in range(max(len(fps), 1))]
    qpad = np.concatenate((np.zeros(shift, dtype=q.dtype), q.ravel()))
    with ctx._temporaries([qpad, xp] + fps + fresh, []) as bufs:
        dq, dx, df, do = bufs[0], bufs[1], bufs[2:2 + len(fps)], bufs[2 + len(fps):]
        fp = (C.c_void_p * max(len(fps), 1))(*[b.ptr for b in df])
        op = (C.c_void_p * len(do))(*[b.ptr + shift * np.dtype(out_dtype).itemsize for b in do])
        rc = ctx.lib.xc_contour_map_dev(ctx.handle, dq.ptr + shift * q.dtype.itemsize, nat.dtype_code(q.dtype), S if nslab is None else nslab, ny, nx,
                                        dx.ptr, xp.shape[-1] if N is None else N, 1 if xp.ndim == 2 else 0, len(fps) if nv is None else nv,
                                        fp, _flags(fps), op, nat.dtype_code(np.dtype(out_dtype)))
        ctx.sync()
        back = [b.download(a.shape, a.dtype) for b, a in zip(do, fresh)]
    for o in back:
        assert (o[:shift] == out_dtype(PAT)).all() and (o[shift + cells:] == out_dtype(PAT)).all(), 'an element outside the plane was written'
    return rc, [o[shift:shift + cells].reshape(S, ny, nx) for o in back]


def check(ctx, q, xp, fps, out_dtype=F64, what='', call=host_call, **kw):
    rc, got = call(ctx, q, xp, fps, out_dtype, **kw)
    assert rc == 0, '%s: status %d (%s)' % (what, rc, ctx.lib.xc_last_error(ctx.handle))
    ref = R.contour_map(q, xp, fps, out_dtype)
    for v, (a, b) in enumerate(zip(got, ref)):
        assert a.dtype == np.dtype(out_dtype)
        same_bits(a, b, '%s vector %d' % (what, v))
    return got


def per_slab_levels(N, nslab, kind='linear'):
    """levels that differ per slab, every other slab decreasing"""
    return np.stack([R.levels(kind, N, decreasing=bool(s % 2)) * (1.0 + 0.5 * s) for s in range(nslab)])


KINDS = ('finite', 'nan', 'inf', 'flat_inf')


# ---------------------------------------------------------------------------------------------------- planes, slabs, dtypes
@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
@pytest.mark.parametrize('nslab', [1, 3])
@pytest.mark.parametrize('plane', R.PLANES, ids=lambda p: '%dx%d' % p)
def test_planes(ctx, plane, nslab, dtype):
    ny, nx = plane
    N = 65
    xp = per_slab_levels(N, nslab)
    fps = [R.values('finite', N, 1), np.stack([R.values('nan', N, 10 + s) for s in range(nslab)])]
    for base in ('smooth', 'noise'):
        q = R.stack(xp, nslab, ny, nx, dtype, base, seed=ny * nx)
        a = check(ctx, q, xp, fps, what='host %s' % base)
        b = check(ctx, q, xp, fps, what='dev %s' % base, call=dev_call)
        for u, v in zip(a, b):
            same_bits(u, v, 'the _dev and the host form')


@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
@pytest.mark.parametrize('cells', [TILE - 1, TILE, TILE + 1, 2 * TILE + 3, 37 * TILE + 1], ids=lambda c: 'cells%d' % c)
def test_tiles_and_workgroups(ctx, cells, dtype):
    """the counts round one tile; 37 tiles and a cell: ten workgroups per slab, each walking three or four tiles, the last one partial.
    Three slabs of an odd cell count, and allocations entered one element in: the head is 0, 1, 2 or 3 cells long"""
    N = 201
    xp = per_slab_levels(N, 3, 'geometric')
    fps = [R.values('finite', N, 2), R.values('inf', N, 3)]
    q = R.stack(xp, 3, 1, cells, dtype, 'noise', seed=cells)
    check(ctx, q, xp, fps, what='host')
    for shift in (0, 1, 2, 3):
        check(ctx, q, xp, fps, what='dev shift %d' % shift, call=dev_call, shift=shift)
    check(ctx, q, xp, fps, F32, what='dev f32 planes', call=dev_call, shift=1)


# ---------------------------------------------------------------------------------------------------- N, nv, shared / per slab
@pytest.mark.parametrize('N,nv', [(n, v) for n in (2, 3, 64, 65, 201) for v in (1, 2, 8)] + [(3000, 1)])
def test_levels_and_vectors_shared_or_per_slab(ctx, N, nv):
    nslab, ny, nx = 3, 5, 257
    if N == 3000:
        ny, nx = 33, 1025                                            # room for every level, and both neighbours of each
    for xs in (False, True):
        xp = per_slab_levels(N, nslab) if xs else R.levels('linear', N, decreasing=True)
        for fs in (False, True):
            fps = [np.stack([R.values(KINDS[v % 4], N, 7 * v + s) for s in range(nslab)]) if fs else R.values(KINDS[v % 4], N, v)
                   for v in range(nv)]
            q = R.stack(xp, nslab, ny, nx, F64, 'noise', seed=N + nv)
            check(ctx, q, xp, fps, what='levels %s vectors %s' % ('per slab' if xs else 'shared', 'per slab' if fs else 'shared'))
    # mixed: the first vector shared, the others per slab
    if nv > 1:
        fps = [R.values('finite', N, 0)] + [np.stack([R.values(KINDS[v % 4], N, v + s) for s in range(nslab)]) for v in range(1, nv)]
        check(ctx, R.stack(xp, nslab, ny, nx, F32, 'smooth', seed=N), xp, fps, what='mixed', call=dev_call)


# ---------------------------------------------------------------------------------------------------- kinds of levels and vectors
@pytest.mark.parametrize('f32', [False, True], ids=['f64levels', 'f32levels'])
@pytest.mark.parametrize('decreasing', [False, True], ids=['inc', 'dec'])
@pytest.mark.parametrize('kind', ['linear', 'geometric', 'gap'])
def test_level_kinds(ctx, kind, decreasing, f32):
    """float32-representable levels run with a float32 tracer (exact hits and float32 neighbours); 'gap' puts the uniform guess more
    than N / 2 levels off for half of the plane, the binary search's ground"""
    N = 201
    xp = R.levels(kind, N, decreasing, f32)
    fps = [R.values(k, N, i) for i, k in enumerate(KINDS)]
    for base in ('smooth', 'noise'):
        q = R.stack(xp, 2, 17, 1023, F32 if f32 else F64, base, seed=5)
        check(ctx, q, xp, fps, what=base)
        check(ctx, q, xp, fps, F32, what=base + ' f32 planes')      # out_dtype f32: the restatement rounded once


def test_every_fallback_is_walked(ctx):
    """the vectors of `values` take numpy's two fall-backs on this plane: asserted on the restatement, so that the bit-for-bit
    comparison above cannot have skipped them"""
    N = 65
    xp = R.levels('linear', N)
    q = R.stack(xp, 1, 33, 1025, F64, 'noise', seed=1)[0].ravel()
    j = np.clip(np.searchsorted(xp, q, side='right') - 1, 0, N - 2)
    inside = (q > xp[0]) & (q < xp[-1]) & (q != xp[j])
    with np.errstate(all='ignore'):
        for kind, want_second, want_third in (('inf', True, False), ('flat_inf', False, True), ('nan', False, False)):
            f = R.values(kind, N)
            slope = (f[j + 1] - f[j]) / (xp[j + 1] - xp[j])
            first = slope * (q - xp[j]) + f[j]
            second = slope * (q - xp[j + 1]) + f[j + 1]
            if want_second:
                assert (inside & np.isnan(first) & ~np.isnan(second)).any()
            if want_third:
                assert (inside & np.isnan(first) & np.isnan(second) & (f[j] == f[j + 1])).any()
            if kind == 'nan':
                assert (inside & np.isnan(f[j]) & ~np.isnan(f[j + 1])).any() and (inside & ~np.isnan(f[j]) & np.isnan(f[j + 1])).any()
                assert (inside & np.isnan(f[j]) & np.isnan(f[j + 1])).any()
    check(ctx, q.reshape(1, 33, 1025), xp, [R.values(k, N) for k in KINDS], what='fall-backs')


def test_all_nan_slab_and_equal_end_levels(ctx):
    """a slab whose first or last level is NaN gets NaN everywhere, its neighbours their own values"""
    N = 64
    xp = per_slab_levels(N, 3)
    xp[1, 0] = np.nan
    fps = [R.values('finite', N), R.values('inf', N)]
    q = R.stack(R.levels('linear', N), 3, 5, 257, F64, 'noise')
    got = check(ctx, q, xp, fps, what='NaN first level')
    assert np.isnan(got[0][1]).all() and np.isnan(got[1][1]).all() and not np.isnan(got[0][2]).all()
    xp[1] = np.nan
    xp[2, -1] = np.nan
    got = check(ctx, q, xp, fps, what='all-NaN levels', call=dev_call)
    assert np.isnan(got[0][1:]).all()


# ---------------------------------------------------------------------------------------------------- limits
def test_lds_limit_on_both_sides(ctx):
    for N, nv, ok in ((4096, 1, True), (4097, 1, False), (910, 8, True), (911, 8, False), (3000, 1, True), (3000, 2, False)):
        xp = R.levels('linear', N)
        fps = [R.values('finite', N, v) for v in range(nv)]
        q = R.stack(xp, 1, 3, 5, F64)
        assert R.refusal(1, N, nv, xp) == (0 if ok else R.XC_EBADARG)
        for call in (host_call, dev_call):
            if ok:
                check(ctx, q, xp, fps, what='N %d nv %d' % (N, nv), call=call)
            else:
                rc, got = call(ctx, q, xp, fps)
                assert rc == nat.XC_EBADARG and all((g == PAT).all() for g in got)


def test_slab_limit_on_both_sides(ctx):
    xp, f = np.array([0.0, 1.0]), np.array([2.0, 4.0])
    q = np.tile(np.array([0.25, 1.5]), (R.MAX_SLABS + 1, 1)).reshape(-1, 1, 2)
    for call in (host_call, dev_call):
        got = check(ctx, q[:R.MAX_SLABS], xp, [f], what='65535 slabs', call=call)
        assert (got[0] == [2.5, 4.0]).all()
        rc, got = call(ctx, q, xp, [f])
        assert rc == nat.XC_EBADARG and (got[0] == PAT).all()


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_planes_alone(ctx):
    N = 5
    xp, f = R.levels('linear', N), R.values('finite', N)
    q = R.stack(xp, 2, 3, 5, F64)

    def refused(rc, got, code=nat.XC_EBADARG):
        assert rc == code, rc
        assert all((g == PAT).all() for g in got)
    for call in (host_call, dev_call):
        refused(*call(ctx, q, xp, [f], N=1))
        refused(*call(ctx, q, xp, [f], nv=0))
        refused(*call(ctx, q, xp, [f] * 8, nv=9))
        refused(*call(ctx, q, xp, [f], nslab=0))
    refused(*host_call(ctx, q, xp, [f], q_code=7))
    refused(*host_call(ctx, q, xp, [f], out_code=-1))
    # null pointers, one at a time, to both entries
    out = np.full(q.size, PAT)
    fp, op, fl = (C.c_void_p * 1)(f.ctypes.data), (C.c_void_p * 1)(out.ctypes.data), (C.c_int * 1)(0)
    nul = (C.c_void_p * 1)(None)
    good = [q.ctypes.data, 1, 2, 3, 5, xp.ctypes.data, N, 0, 1, fp, fl, op, 1]
    for fn in (ctx.lib.xc_contour_map, ctx.lib.xc_contour_map_dev):
        for at, bad in ((0, None), (5, None), (9, None), (10, None), (11, None), (9, nul), (11, nul)):
            a = list(good)
            a[at] = bad
            assert fn(ctx.handle, *a) == nat.XC_EBADARG
        assert fn(None, *good) == nat.XC_EBADARG
    ctx.sync()
    assert (out == PAT).all()
    # the host form reads the levels first: adjacent equal levels under the reference's text, a slab out of order
    xe = xp.copy()
    xe[2] = xe[1]
    refused(*host_call(ctx, q, xe, [f]), code=nat.XC_EEDGES)
    assert ctx.lib.xc_last_error(ctx.handle) == b'non monotonic bins'
    xe = np.stack([xp, xp[::-1]])
    xe[1, 1], xe[1, 2] = xe[1, 2], xe[1, 1]
    refused(*host_call(ctx, q, xe, [f]))
    xe = xp.copy()
    xe[2] = np.inf
    refused(*host_call(ctx, q, xe, [f]))
    for x in (xe, np.stack([xp, xp[::-1]])):
        assert R.refusal(2, N, 1, x) == (R.XC_EBADARG if x is xe else 0)
