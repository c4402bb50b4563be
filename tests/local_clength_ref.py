"""numpy restatement of the sliding-window contour lengths of K11 (xc_lclen.hip) -- a helper for the tests, no tests here.

Windows are centred on the nodes 0, s, 2 s, ... of each plane dim, own the nodes [centre - w // 2, centre - w // 2 + w - 1] and are
clipped to the plane.  A window's level is given or its NaN-skipping mean in float64, summed in the kernel's order: per row left to
right from 0.0, the row sums top to bottom, one division by the valid count (np.cumsum is sequential, so its last element is that
sum).  A window's length is clength_ref.contour_lengths on the cropped plane with the cropped coordinates.
"""
import numpy as np

import clength_ref as CR


def centres(n, s):
    return np.arange(0, n, s)


def bounds(n, w, s):
    """-> (first node, last node) of every window along a dim of n nodes, both inclusive, clipped"""
    lo = centres(n, s) - w // 2
    return np.maximum(lo, 0), np.minimum(lo + w - 1, n - 1)


def sequential_mean(win, min_periods):
    """the NaN-skipping mean of a 2-D window in the kernel's order; NaN with fewer than min_periods valid nodes"""
    win = np.asarray(win, dtype=np.float64)
    ok = ~np.isnan(win)
    rows = np.cumsum(np.where(ok, win, 0.0), axis=1)[:, -1]          # left to right, from 0.0 (a NaN node adds 0.0: nothing)
    tot = np.cumsum(rows)[-1]                                          # top to bottom
    n = int(ok.sum())
    if n < min_periods:
        return np.nan
    with np.errstate(invalid='ignore', divide='ignore'):
        return float(np.float64(tot) / np.float64(n))


def window_levels(q2d, window, stride, min_periods=None):
    """-> (nwy, nwx) float64: every window's sequential mean"""
    (wy, wx), (sy, sx) = window, stride
    ny, nx = q2d.shape
    mp = wy * wx if min_periods is None else min_periods
    (r0, r1), (c0, c1) = bounds(ny, wy, sy), bounds(nx, wx, sx)
    out = np.empty((r0.size, c0.size))
    for a in range(r0.size):
        for b in range(c0.size):
            out[a, b] = sequential_mean(q2d[r0[a]:r1[a] + 1, c0[b]:c1[b] + 1], mp)
    return out


def window_length(q2d, level, ycoord, xcoord, window, stride, wj, wi, latlon=False):
    """-> (total, segment count) of window (wj, wi) at `level`"""
    (wy, wx), (sy, sx) = window, stride
    ny, nx = q2d.shape
    (r0, r1), (c0, c1) = bounds(ny, wy, sy), bounds(nx, wx, sx)
    sub = np.asarray(q2d[r0[wj]:r1[wj] + 1, c0[wi]:c1[wi] + 1], dtype=np.float64)
    t, n = CR.contour_lengths(sub, [level], ycoord[r0[wj]:r1[wj] + 1], xcoord[c0[wi]:c1[wi] + 1], latlon)
    return t[0], n[0]


def local_contour_lengths(q2d, levels, ycoord, xcoord, window, stride, latlon=False, sample=None):
    """-> (totals f64 (nwy, nwx), counts int64 (nwy, nwx)) of one slab; levels (nwy, nwx) or a scalar.  `sample`: a list of
    (wj, wi) -- only those windows are computed, the others hold NaN / -1"""
    (wy, wx), (sy, sx) = window, stride
    ny, nx = q2d.shape
    nwy, nwx = centres(ny, sy).size, centres(nx, sx).size
    lv = np.broadcast_to(np.asarray(levels, dtype=np.float64), (nwy, nwx))
    tot = np.full((nwy, nwx), np.nan)
    cnt = np.full((nwy, nwx), -1, dtype=np.int64)
    todo = sample if sample is not None else [(a, b) for a in range(nwy) for b in range(nwx)]
    for a, b in todo:
        tot[a, b], cnt[a, b] = window_length(q2d, lv[a, b], ycoord, xcoord, window, stride, a, b, latlon)
    return tot, cnt
