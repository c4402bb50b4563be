"""Restatement of K13 (xc_cpiece.hip: the connected pieces of a contour and their statistics) -- a helper for the tests, no tests
here.

Segments and the walk: contour_join_ref (plain plane) / contour_join_periodic_ref (periodic X) -- `segments` and `join`.  A piece is
one joined polyline, dropped ones INCLUDED (a piece whose segments all have coincident end points stays, with length 0).
Coordinates: np.interp(row, arange(ny), ycoord) and np.interp(column, arange(nx), xcoord), on a periodic plane
np.interp(column, arange(nx + 1), [xcoord..., xcoord[0] + period]) (clength_periodic_ref.extend_plane).  ycoord / xcoord are what the
library receives: float64, radians with latlon.
Per piece, in plain Python:
  length   math.fsum of clength_ref's segment lengths (haversine or hypot) over the segments whose end points differ, times RADIUS
           with latlon
  area     math.fsum of 0.5 * ((Ya' + Yb') * (Xa - Xb)) over the directed segments a -> b, Y' = sin(Y) and times RADIUS^2 with latlon;
           NaN for an open piece.  `area_abs` is math.fsum of the |terms| (same scaling): the scale of the cancelling sum.
  winding  of a ring: over the links i -> next(i) of the walk, the closing link included, +1 where c2[i] == nx and c1[next] == 0,
           -1 where c2[i] == 0 and c1[next] == nx; 0 for an open piece and on a plain plane
  nseg, closed, first_edge (the smallest e_from), row_min / row_max (over both end points of every segment) by direct count.
Sign of the area (both coordinates ascending): S > 0 for a ring that encloses values ABOVE the level, S < 0 for one that encloses
values below it; each descending coordinate flips the sign.
"""
import math

import numpy as np

import clength_ref as CR
import contour_join_ref as JR
import contour_join_periodic_ref as JP

RADIUS = CR.RADIUS

DTYPE = np.dtype([('first_edge', np.int64), ('nseg', np.int64), ('closed', np.bool_), ('winding', np.int32),
                  ('length', np.float64), ('area', np.float64), ('row_min', np.float64), ('row_max', np.float64),
                  ('area_abs', np.float64)])


def pieces(q2d, levels, ycoord, xcoord, latlon=False, period=None):
    """one plane -> per level (in the order given; a NaN level has none) a structured array (DTYPE), one row per piece, ordered
    by first_edge.  period: None (plain plane) or the X period (periodic plane)."""
    q = np.asarray(q2d, dtype=np.float64)
    ny, nx = q.shape
    y = np.asarray(ycoord, dtype=np.float64)
    x = np.asarray(xcoord, dtype=np.float64)
    ring_plane = period is not None
    xe = np.concatenate([x, [x[0] + np.float64(period)]]) if ring_plane else x
    yi, xi = np.arange(ny), np.arange(xe.size)
    out = []
    for ef, et, pts in (JP.segments(q, levels) if ring_plane else JR.segments(q, levels)):
        rows = []
        if ef.size:
            Y1, Y2 = np.interp(pts[:, 0], yi, y), np.interp(pts[:, 2], yi, y)
            X1, X2 = np.interp(pts[:, 1], xi, xe), np.interp(pts[:, 3], xi, xe)
            ln = CR.haversine(X1, Y1, X2, Y2) if latlon else np.hypot(X1 - X2, Y1 - Y2)
            differ = ~((pts[:, 0] == pts[:, 2]) & (pts[:, 1] == pts[:, 3]))
            ya, yb = (np.sin(Y1), np.sin(Y2)) if latlon else (Y1, Y2)
            terms = 0.5 * ((ya + yb) * (X1 - X2))
            for segs, closed in JR.join(ef, et):
                segs = np.asarray(segs)
                length = math.fsum(ln[segs][differ[segs]])
                S = math.fsum(terms[segs])
                Sabs = math.fsum(np.abs(terms[segs]))
                if latlon:
                    length, S, Sabs = length * RADIUS, S * (RADIUS * RADIUS), Sabs * (RADIUS * RADIUS)
                w = 0
                if closed and ring_plane:
                    for a, b in zip(segs, np.roll(segs, -1)):
                        if pts[a, 3] == nx and pts[b, 1] == 0:
                            w += 1
                        elif pts[a, 3] == 0 and pts[b, 1] == nx:
                            w -= 1
                rr = pts[segs][:, [0, 2]]
                rows.append((int(ef[segs].min()), segs.size, bool(closed), w, length, S if closed else np.nan,
                             float(rr.min()), float(rr.max()), Sabs))
        rows.sort(key=lambda t: t[0])
        out.append(np.array(rows, dtype=DTYPE))
    return out


def stack_pieces(q, levels, ycoord, xcoord, latlon=False, period=None):
    """a stack (nslab, ny, nx) -> out[slab][k]; levels (N,) or (nslab, N)"""
    q = np.asarray(q)
    lv = np.asarray(levels, dtype=np.float64)
    return [pieces(q[s], lv[s] if lv.ndim == 2 else lv, ycoord, xcoord, latlon, period) for s in range(q.shape[0])]
