# -*- coding: utf-8 -*-
"""K26 (xc_coarsen, xc_contour_lengths_scales) restated in numpy: the rule of include/xcontour_hip.h, K26 section, with loops over
the r block columns and rows only.  Beside it the deliberately WRONG rules the tests must be able to tell from it (`wrong`), the
refusals, and the fixed inputs the host and the gpu tests share."""
import warnings

import numpy as np

XC_OK, XC_EBADARG, XC_EEDGES = 0, -1, -2
MAXR, MAXRATIO = 8, 64
NAN, INF = np.nan, np.inf


# ---------------------------------------------------------------------------------------------------- the rule
def _blocks(q, r):
    q = np.asarray(q).astype(np.float64)
    cy, cx = q.shape[-2] // r, q.shape[-1] // r
    return q[..., :cy * r, :cx * r].reshape(q.shape[:-2] + (cy, r, cx, r))


def coarsen(q, r, skipna=False):
    """(..., ny, nx) f32 / f64 -> float64 (..., ny // r, nx // r): every block summed row by row, each row left to right FROM its
    first value, the row sums top to bottom FROM the first, divided once by r * r.  skipna: NaN nodes are left out of the same
    order, a row with none adds nothing, the divisor is the number of nodes used, a block with none is NaN"""
    b = _blocks(q, r)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        if not skipna:
            tot = None
            for dr in range(r):
                row = b[..., :, dr, :, 0].copy()
                for dc in range(1, r):
                    row = row + b[..., :, dr, :, dc]
                tot = row if tot is None else tot + row
            return tot / float(r * r)
        shape = b.shape[:-4] + (b.shape[-4], b.shape[-2])
        tot, have, n = np.zeros(shape), np.zeros(shape, dtype=bool), np.zeros(shape, dtype=np.int64)
        for dr in range(r):
            row, rhave = np.zeros(shape), np.zeros(shape, dtype=bool)
            for dc in range(r):
                x = b[..., :, dr, :, dc]
                ok = ~np.isnan(x)
                row = np.where(ok, np.where(rhave, row + x, x), row)
                rhave |= ok
                n += ok
            tot = np.where(rhave, np.where(have, tot + row, row), tot)
            have |= rhave
        return np.where(n > 0, tot / np.where(n > 0, n, 1).astype(np.float64), NAN)


def coarsen_coords(c, r):
    """float64 coordinates -> the sequential block means, float64; nothing is cast"""
    b = np.asarray(c, dtype=np.float64)
    b = b[:b.size // r * r].reshape(-1, r)
    s = b[:, 0].copy()
    for k in range(1, r):
        s = s + b[:, k]
    return s / float(r)


def refusal(ny, nx, ratios, periodic=False, lengths=True):
    """the status of a call on a (ny, nx) plane with these ratios, shapes and ratios alone considered"""
    if lengths and not 1 <= len(ratios) <= MAXR:
        return XC_EBADARG
    for r in ratios:
        if not 1 <= r <= MAXRATIO:
            return XC_EBADARG
        if not lengths:
            if ny // r < 1 or nx // r < 1:
                return XC_EBADARG
            continue
        if ny // r < 2 or (periodic and nx % r) or (not periodic and nx // r < 2):
            return XC_EBADARG
    return XC_OK


# ---------------------------------------------------------------------------------------------------- wrong rules
WRONG_PLANE = ('pairwise', 'column_first', 'skipna_rr', 'pad')
WRONG_COORD = ('first_node', 'f32_coords')


def wrong(kind, q, r, skipna=False):
    """a coarse plane under one wrong rule"""
    b = _blocks(q, r)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        if kind == 'pairwise':                  # np.mean / np.nanmean: numpy's pairwise, unrolled sums over the merged block
            m = np.moveaxis(b, -3, -2).reshape(b.shape[:-4] + (b.shape[-4], b.shape[-2], r * r))
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)        # (nanmean of an all-NaN block)
                return np.nanmean(m, axis=-1) if skipna else m.mean(axis=-1)
        if kind == 'column_first':              # each block column summed top to bottom, the column sums left to right
            return np.swapaxes(coarsen(np.swapaxes(np.asarray(q), -1, -2), r, skipna), -1, -2)
        if kind == 'skipna_rr':                 # skipna, but divided by r * r whatever was used
            n = (~np.isnan(b)).sum(axis=(-3, -1))
            return coarsen(q, r, True) * n / float(r * r)
        if kind == 'pad':                       # trailing partial blocks kept: padded with NaN and averaged over what is there
            q = np.asarray(q).astype(np.float64)
            py, px = -q.shape[-2] % r, -q.shape[-1] % r
            qp = np.pad(q, [(0, 0)] * (q.ndim - 2) + [(0, py), (0, px)], constant_values=NAN)
            full = coarsen(qp, r, True)
            if not skipna:                      # (inside the plane the NaN rule of the call)
                plain = coarsen(q, r, False)
                full[..., :plain.shape[-2], :plain.shape[-1]] = plain
            return full
    raise ValueError(kind)


def wrong_coords(kind, c, r):
    c = np.asarray(c, dtype=np.float64)
    if kind == 'first_node':
        return c[:c.size // r * r:r].copy()
    if kind == 'f32_coords':
        return coarsen_coords(c, r).astype(np.float32).astype(np.float64)
    raise ValueError(kind)


# ---------------------------------------------------------------------------------------------------- inputs
def field(nslab, ny, nx, dtype=np.float64, seed=0):
    """values of mixed magnitude, so that the order of a sum shows in its last bits: (-1)^i 10^(2 (i mod 7) - 6) over the flat
    index, scaled by a hashed factor in [1, 2) and by a smooth field in [0.5, 1.5] (a factor, not a term: added, it would swallow
    the small values of a float32 tracer).  Twelve decades: more than the 29 bits a float64 sum has to spare over float32 terms, so
    the order shows for a float32 tracer too"""
    i = np.arange(nslab * ny * nx, dtype=np.int64).reshape(nslab, ny, nx)
    h = ((i.astype(np.uint64) * np.uint64(2654435761) + np.uint64(seed * 977 + 12345)) % np.uint64(1 << 20)).astype(np.float64) / (1 << 20)
    spikes = np.where(i % 2 == 0, 1.0, -1.0) * 10.0 ** (2 * (i % 7) - 6) * (1.0 + h)
    y, x = np.arange(ny)[:, None] / max(ny - 1, 1), np.arange(nx)[None, :] / max(nx - 1, 1)
    smooth = 1.0 + 0.5 * np.sin(3.0 * y + 0.5 * seed) * np.cos(5.0 * x)
    return (spikes * smooth[None] * (1.0 + 0.1 * np.arange(nslab)[:, None, None])).astype(dtype)


def with_specials(q, r):
    """`q` with, in blocks of ratio `r` that exist in it: a NaN at a block's first node, at a block's last node, a block whose only
    finite node is its last, an all-NaN block row, an all-NaN block, +inf in one block, -inf and +inf in another.  Needs at least
    3 x 3 blocks (fewer: only what fits)"""
    q = q.copy()
    cy, cx = q.shape[-2] // r, q.shape[-1] // r

    def blk(I, J):
        return q[..., I * r:(I + 1) * r, J * r:(J + 1) * r] if I < cy and J < cx else None
    for (I, J), what in (((0, 0), 'first'), ((0, 1), 'last'), ((1, 0), 'only_last'), ((1, 1), 'row'), ((0, 2), 'all'),
                         ((2, 0), 'inf'), ((2, 1), 'infs'), ((1, 2), 'only_first')):
        b = blk(I, J)
        if b is None:
            continue
        if what == 'first':
            b[..., 0, 0] = NAN
        elif what == 'last':
            b[..., r - 1, r - 1] = NAN
        elif what == 'only_last':
            keep = b[..., r - 1, r - 1].copy(); b[...] = NAN; b[..., r - 1, r - 1] = keep
        elif what == 'only_first':
            keep = b[..., 0, 0].copy(); b[...] = NAN; b[..., 0, 0] = keep
        elif what == 'row':
            b[..., r // 2, :] = NAN
        elif what == 'all':
            b[...] = NAN
        elif what == 'inf':
            b[..., 0, r - 1] = INF
        elif what == 'infs':
            b[..., 0, 0] = -INF; b[..., r - 1, 0] = INF
    return q


def coords(n, salt, scale=1.0):
    """float32-representable, unevenly spaced, ascending coordinates in float64 (what the facade hands K10 with latlon=False);
    their block sums are not exact in float32 and their block means differ from the first node's"""
    i = np.arange(n, dtype=np.uint64)
    h = ((i * np.uint64(40503) + np.uint64(salt * 97 + 1)) * np.uint64(2246822519) % np.uint64(1 << 24)).astype(np.float64) / (1 << 24)
    return np.cumsum(scale * (1.0 + 0.5 * h)).astype(np.float32).astype(np.float64)


def levels(q, N):
    """N ascending levels inside the range of the finite values of the coarsest plane worth tracing"""
    f = q[np.isfinite(q)].astype(np.float64)
    lo, hi = np.percentile(f, 20), np.percentile(f, 80)
    return np.linspace(lo, hi, N)
