"""numpy restatement of the periodic X direction of K10 / K11 (xc_contour_lengths_periodic, xc_local_contour_lengths_periodic) -- a
helper for the tests, no tests here.

The rule.  `period` is a float64: finite, non-zero, of the sign of xcoord[nx-1] - xcoord[0], |period| > |xcoord[nx-1] - xcoord[0]|;
the ring needs nx >= 2.  The coordinate of a node column c outside [0, nx) is xcoord[c mod nx] + period or xcoord[c mod nx] - period,
one float64 addition or subtraction.  Y never wraps.
  K10: the plane gains one cell column, index nx-1, between node column nx-1 (cL = nx-1, xL = xcoord[nx-1]) and node column 0 one
    period on (xR = xcoord[0] + period); everything else is K10's rule (clength_ref).  That is K10 on extend_plane().
  K11: window i owns the node columns [i - wx/2, i - wx/2 + wx - 1] modulo nx, in that unwrapped order with the unwrapped
    coordinates; wx <= nx; Y clipping, centres and nwx = ceil(nx / sx) as before; the mean per row left to right in window order.
    That is K11 (local_clength_ref) on tile_plane() -- h columns of the ring copied to either side, h a multiple of sx and >= wx --
    at the centres h/sx ... h/sx + nwx - 1.
"""
import numpy as np

import clength_ref as CR
import local_clength_ref as LR


def check_period(x, period):
    x = np.asarray(x, dtype=np.float64)
    span = x[-1] - x[0]
    assert x.size >= 2 and np.isfinite(period) and period != 0 and period * span >= 0 and abs(period) > abs(span)


def extend_plane(q, x, period):
    """-> (q with column 0 appended as column nx, x with x[0] + period appended); q (..., ny, nx)"""
    q, x = np.asarray(q), np.asarray(x, dtype=np.float64)
    check_period(x, period)
    return np.concatenate([q, q[..., :1]], axis=-1), np.concatenate([x, [x[0] + np.float64(period)]])


def tile_plane(q, x, period, h):
    """-> (q, x) with h columns of the ring copied to either side: node columns -h ... nx + h - 1, column c holding q[..., c mod nx]
    at x[c mod nx] + lap * period, lap = floor(c / nx) (lap = -1: x - period, exactly)"""
    q, x = np.asarray(q), np.asarray(x, dtype=np.float64)
    check_period(x, period)
    nx = x.size
    c = np.arange(-h, nx + h)
    lap = np.floor_divide(c, nx)
    xm = x[c % nx]
    xt = np.where(lap == 0, xm, np.where(lap == 1, xm + np.float64(period), np.where(lap == -1, xm - np.float64(period),
                                                                                     xm + lap * np.float64(period))))
    return q[..., c % nx], xt


def halo(wx, sx):
    """the smallest multiple of sx that is >= wx"""
    return -(-wx // sx) * sx


def contour_lengths(q2d, levels, ycoord, xcoord, period, latlon=False):
    """periodic K10 of one slab -> (totals f64 (N,), segment counts int64 (N,))"""
    qe, xe = extend_plane(q2d, xcoord, period)
    return CR.contour_lengths(qe, levels, ycoord, xe, latlon)


def contour_lengths_fast(q2d, levels, ycoord, xcoord, period, latlon=False):
    qe, xe = extend_plane(q2d, xcoord, period)
    return CR.contour_lengths_fast(qe, levels, ycoord, xe, latlon)


def window_levels(q2d, window, stride, period_x, min_periods=None):
    """-> (nwy, nwx) float64: every periodic window's sequential mean (period_x: any valid period; the coordinates play no part)"""
    nx = q2d.shape[1]
    assert window[1] <= nx
    h = halo(window[1], stride[1])
    qt, _ = tile_plane(q2d, np.arange(nx, dtype=np.float64), float(nx), h)
    lv = LR.window_levels(qt, window, stride, min_periods)
    a = h // stride[1]
    return lv[:, a:a + LR.centres(nx, stride[1]).size]


def local_contour_lengths(q2d, levels, ycoord, xcoord, period, window, stride, latlon=False, sample=None):
    """periodic K11 of one slab -> (totals f64 (nwy, nwx), counts int64 (nwy, nwx)); levels (nwy, nwx) or a scalar.  `sample`: a list
    of (wj, wi) -- only those windows are computed, the others hold NaN / -1"""
    nx = q2d.shape[1]
    assert window[1] <= nx
    sx = stride[1]
    h = halo(window[1], sx)
    qt, xt = tile_plane(q2d, xcoord, period, h)
    nwy, nwx = LR.centres(q2d.shape[0], stride[0]).size, LR.centres(nx, sx).size
    a = h // sx
    nwt = LR.centres(nx + 2 * h, sx).size
    lv = np.full((nwy, nwt), np.nan)
    lv[:, a:a + nwx] = np.broadcast_to(np.asarray(levels, dtype=np.float64), (nwy, nwx))
    todo = sample if sample is not None else [(j, i) for j in range(nwy) for i in range(nwx)]
    tot, cnt = LR.local_contour_lengths(qt, lv, ycoord, xt, window, stride, latlon, sample=[(j, a + i) for j, i in todo])
    return tot[:, a:a + nwx], cnt[:, a:a + nwx]
