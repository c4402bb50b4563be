"""numpy restatement of the sliding-window contour lengths of K11 (xc_lclen.hip) -- a helper for the tests, no tests here.

Windows are centred on the nodes 0, s, 2 s, ... of each plane dim, own the nodes [centre - w // 2, centre - w // 2 + w - 1] and are
clipped to the plane.  A window's level is given or its NaN-skipping mean in float64, summed in the kernel's order: per row left to
right from 0.0, the row sums top to bottom from 0.0, one division by the valid count (np.cumsum is sequential and starts from its
first element, so a 0.0 goes in front; its last element is then that sum).  A window's length is clength_ref.contour_lengths on the
cropped plane with the cropped coordinates.
"""
import numpy as np

import clength_ref as CR

# the launch constants of xc_lclen.hip that launch_shape restates
LCLEN_SMALL = 2048        # LCLEN_SMALL: an unclipped window of up to this many cells runs on one wave (64 threads), else on four (256)
LCLEN_RB = 16             # LCLEN_RB: cell rows of a strip
LCLEN_LANES = 64          # cell columns of a strip: one per lane of a wave
LCLEN_STRIPS = 31         # LCLEN_STRIPS = 32767 // (64 * 16): strips a wave takes between two carries


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
    # left to right, from an explicit 0.0 (a NaN node adds 0.0: nothing; 0.0 + -0.0 is +0.0: a sum is never -0.0)
    rows = np.cumsum(np.concatenate([np.zeros((win.shape[0], 1)), np.where(ok, win, 0.0)], axis=1), axis=1)[:, -1]
    tot = np.cumsum(np.concatenate([[0.0], rows]))[-1]                 # top to bottom, from 0.0
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


def launch_shape(window, plane_shape, clipped_rows, clipped_cols):
    """the launch rule of launch_local_contour_lengths / lclen_window (xc_lclen.hip), restated -> (threads per block, rounds of the
    mean loop, strips of the window, rounds of the carry loop).  The threads follow from the UNCLIPPED window (on a ring no window is
    clipped in X, and wx <= nx: the same expression); the rest from the window as clipped: `clipped_rows` x `clipped_cols` nodes.
    The mean loop runs only where no level is given, the carry loop only where the level is not NaN."""
    (wy, wx), (ny, nx) = window, plane_shape
    threads = 64 if (min(wy, ny) - 1) * (min(wx, nx) - 1) <= LCLEN_SMALL else 256
    mean_rounds = -(-clipped_rows // threads)
    ch, cw = clipped_rows - 1, clipped_cols - 1
    strips = -(-ch // LCLEN_RB) * -(-cw // LCLEN_LANES) if ch > 0 and cw > 0 else 0
    carry_rounds = -(-strips // (threads // 64 * LCLEN_STRIPS))
    return threads, mean_rounds, strips, carry_rounds


def det_window_total(q2d, level, ycoord, xcoord, window, stride, wj, wi, latlon=False):
    """K11's sum of window (wj, wi) at `level`, modelled: the segment lengths of the cropped window through the oracle's fixed-point
    rule (deterministic_bin_sums, 4 limbs) on the window top of clen_bound over the WHOLE plane's coordinates (not the crop's: the
    header of xc_lclen.hip), times the radius on the sphere, NaN for a total of 0 or a NaN level -> float"""
    import xcontour_oracle as O
    if np.isnan(level):
        return np.nan
    (wy, wx), (sy, sx) = window, stride
    ny, nx = q2d.shape
    (r0, r1), (c0, c1) = bounds(ny, wy, sy), bounds(nx, wx, sx)
    sub = np.asarray(q2d[r0[wj]:r1[wj] + 1, c0[wi]:c1[wi] + 1], dtype=np.float64)
    k, *_, ln = CR.segments_fast(sub, [level], ycoord[r0[wj]:r1[wj] + 1], xcoord[c0[wi]:c1[wi] + 1], latlon)
    t = float(O.deterministic_bin_sums(k + 1, ln, 1, top=O.det_window_top(CR.clen_bound(ycoord, xcoord, latlon)), nlimb=4)[0])
    return np.nan if t == 0 else (t * CR.RADIUS if latlon else t)
