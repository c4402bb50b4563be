# -*- coding: utf-8 -*-
"""K25 (xc_contour_map) restated: the rule of include/xcontour_hip.h in numpy, its refusals, deliberately wrong variants of it, and
the inputs the gpu tests run (test_gpu_cmap_records.py); test_cmap_host.py pins all of this without a GPU.  No tests here."""
import numpy as np

XC_OK, XC_EBADARG, XC_EEDGES = 0, -1, -2
MAXV, MAX_LDS_DOUBLES, MAX_SLABS = 8, 8192, 65535

# the planes of the gpu tests: odd cell counts put slabs 1 and 2 off the 16-byte grid, so head and tail paths run in every slab
PLANES = ((1, 1), (1, 7), (3, 5), (2, 129), (5, 255), (5, 256), (5, 257), (17, 1023), (33, 1025))


def _slab(a, s):
    a = np.asarray(a, dtype=np.float64)
    return a[s] if a.ndim == 2 else a


def contour_map(q, xp, fps, out_dtype=np.float64):
    """THE RULE.  q (nslab, ny, nx) f32/f64, xp (N,) or (nslab, N), fps a sequence of (N,) / (nslab, N) -> a list of planes: per slab
    np.interp(q, X, F) on float64, X, F reversed when not xp[0] < xp[-1] (reference core.py:1426-1430); a slab whose first or last
    level is NaN gives NaN; the float64 result is rounded once to `out_dtype`."""
    q = np.asarray(q)
    outs = [np.empty(q.shape, dtype=np.float64) for _ in fps]
    for s in range(q.shape[0]):
        x, qs = _slab(xp, s), q[s].astype(np.float64)
        rev = not (x[0] < x[-1])
        for v, fp in enumerate(fps):
            f = _slab(fp, s)
            if np.isnan(x[0]) or np.isnan(x[-1]):
                outs[v][s] = np.nan
            else:
                outs[v][s] = np.interp(qs, x[::-1], f[::-1]) if rev else np.interp(qs, x, f)
    return [o.astype(out_dtype) for o in outs]


def refusal(nslab, N, nv, xp=None, q_dtype=np.float64, out_dtype=np.float64, host=True):
    """the status a call returns before anything is written; `xp`: the levels, read by the host form only"""
    if nslab < 1 or N < 2 or not 1 <= nv <= MAXV or nslab > MAX_SLABS or (nv + 1) * N > MAX_LDS_DOUBLES:
        return XC_EBADARG
    if np.dtype(q_dtype) not in (np.dtype(np.float32), np.dtype(np.float64)) or np.dtype(out_dtype) not in (np.dtype(np.float32), np.dtype(np.float64)):
        return XC_EBADARG
    if host and xp is not None:
        x = np.asarray(xp, dtype=np.float64).reshape(-1, N)
        x = x[~(np.isnan(x[:, 0]) | np.isnan(x[:, -1]))]
        d = np.diff(x, axis=1)
        if (d == 0).any():
            return XC_EEDGES
        if not np.isfinite(x).all() or not np.where(x[:, :1] < x[:, -1:], d > 0, d < 0).all():
            return XC_EBADARG
    return XC_OK


def interp_steps(x, X, F, clamp=True, hit_right=False, ft=np.float64):
    """numpy's arr_interp step by step for ascending X (what interp_locate / interp_eval run on the device); the flags make it WRONG:
    clamp=False extrapolates past the ends, hit_right takes F[j + 1] at an exact hit x == X[j], ft=float32 does the arithmetic there"""
    x, X, F = np.asarray(x).astype(ft), np.asarray(X).astype(ft), np.asarray(F).astype(ft)
    n = len(X)
    with np.errstate(all='ignore'):
        j = np.searchsorted(X, x, side='right') - 1
        jj = np.clip(j, 0, n - 2)
        slope = (F[jj + 1] - F[jj]) / (X[jj + 1] - X[jj])
        r = slope * (x - X[jj]) + F[jj]
        r2 = slope * (x - X[jj + 1]) + F[jj + 1]
        r = np.where(np.isnan(r), r2, r)
        r = np.where(np.isnan(r) & (F[jj + 1] == F[jj]), F[jj], r)
        inside = (x >= X[0]) & (x <= X[-1])
        r = np.where(inside & (x == X[jj]), F[jj + 1] if hit_right else F[jj], r)
        r = np.where(x == X[-1], F[-1], r)
        if clamp:
            r = np.where(x > X[-1], F[-1], np.where(x < X[0], F[0], r))
        r = np.where(np.isnan(x), x, r)
    return r.astype(np.float64)


def variant(q, xp, fps, **flags):
    """contour_map through interp_steps; flags: those of interp_steps, and reversal=False -- the direction of the levels ignored"""
    reversal = flags.pop('reversal', True)
    q = np.asarray(q)
    outs = [np.empty(q.shape, dtype=np.float64) for _ in fps]
    for s in range(q.shape[0]):
        x, qs = _slab(xp, s), q[s].astype(np.float64)
        rev = reversal and not (x[0] < x[-1])
        for v, fp in enumerate(fps):
            f = _slab(fp, s)
            outs[v][s] = np.nan if np.isnan(x[0]) or np.isnan(x[-1]) else interp_steps(qs, x[::-1] if rev else x, f[::-1] if rev else f, **flags)
    return outs


# ---------------------------------------------------------------------------------------------------- inputs of the gpu tests
def levels(kind, N, decreasing=False, f32=False):
    """N strictly increasing finite levels: 'linear'; 'geometric' spacing; 'gap' -- N - 1 levels in [0, 1] and one at 1e6, so that the
    uniform guess of a node in [0, 1] is level 0 whatever its bracket: wrong by more than N / 2"""
    if kind == 'linear':
        x = np.linspace(-1.25, 2.5, N)
    elif kind == 'geometric':
        x = np.geomspace(1e-3, 1e3, N) - 1.0
    elif kind == 'gap':
        x = np.concatenate((np.linspace(0.0, 1.0, N - 1), [1e6])) if N > 2 else np.array([0.0, 1e6])
    else:
        raise ValueError(kind)
    if f32:
        x = x.astype(np.float32).astype(np.float64)
    assert (np.diff(x) > 0).all()
    return x[::-1].copy() if decreasing else x


def values(kind, N, seed=0):
    """a value vector: 'finite'; 'nan' -- an isolated NaN (its two brackets have it at j + 1 and at j) and two adjacent ones (a bracket
    with both); 'inf' -- +inf and -inf; 'flat_inf' -- two adjacent +inf: equal ends with a NaN slope, numpy's last fall-back"""
    f = np.random.default_rng(1000 + seed).standard_normal(N) * 3.0
    if kind == 'finite':
        return f
    a = N // 3
    if kind == 'nan':
        f[a] = np.nan
        if N >= 6:
            f[N - 3] = f[N - 2] = np.nan
    elif kind == 'inf':
        f[a] = np.inf
        f[N - 1 - a if N - 1 - a != a else N - 1] = -np.inf
    elif kind == 'flat_inf':
        f[a] = np.inf
        f[min(a + 1, N - 1)] = np.inf
    else:
        raise ValueError(kind)
    return f


def tracer(X, ncell, dtype, base='noise', seed=0):
    """`ncell` tracer values against the levels X (either direction).  First every special value that fits -- each level exactly, its
    two neighbours (nextafter in the tracer's dtype), values below the first and above the last level, NaN, +inf, -inf, -0.0 --,
    then the base: 'smooth' (neighbouring lanes share a bracket) or white 'noise' (they never do), both reaching past the ends"""
    rng = np.random.default_rng(seed)
    X = np.asarray(X, dtype=np.float64)
    lo, hi = X.min(), X.max()
    span = hi - lo
    if base == 'smooth':
        q = lo + span * (0.5 + 0.55 * np.sin(np.linspace(0.0, 9.0, ncell)))
    else:
        q = rng.uniform(lo - 0.05 * span, hi + 0.05 * span, ncell)
    q = q.astype(dtype)
    Xd = X.astype(dtype)
    sp = np.concatenate(([np.nan, np.inf, -np.inf, -0.0, lo - 1.0, hi + 1.0, lo - span, hi + span], X)).astype(dtype)
    sp = np.concatenate((sp, np.nextafter(Xd, dtype(-np.inf)), np.nextafter(Xd, dtype(np.inf))))
    k = min(ncell, sp.size)
    q[:k] = sp[:k]
    return q


def stack(xp, nslab, ny, nx, dtype, base='noise', seed=0):
    """(nslab, ny, nx) tracer for levels xp (N,) or (nslab, N): slab s built against its own levels; slab 1 starts its specials with
    the levels themselves rolled to the front, so that small planes see hits too"""
    q = np.empty((nslab, ny * nx), dtype=dtype)
    for s in range(nslab):
        t = tracer(_slab(xp, s), ny * nx, dtype, base, seed + s)
        q[s] = np.roll(t, -8 * (s % 2)) if ny * nx > 16 else t
    return q.reshape(nslab, ny, nx)
