"""numpy restatement of the line-integral rule of K15 (xc_cline.hip) on top of clength_ref.segments_fast -- a helper for the
tests, no tests here.

The rule (float64 throughout).  Segments are K10's (clength_ref): cells, crossed levels, cases, saddle pairing, end points in
index space, their mapping to coordinates and the length `len`; segments with coincident end points dropped.  Every end point
lies on a grid edge between two nodes, and F(u) is the integrand mapped onto it as the coordinates are: on a node that node's
value (the other node does not enter), else (F1 - F0) * (x - i0) + F0 with (i0, F0) the edge's first node -- the left one of a
top / bottom edge, the upper one of a left / right edge.  term = (0.5 * (F(u) + F(v))) * len.  A segment with a NaN F(u) or
F(v) is skipped: no length, no term, no count.  Per level: length = sum of len, integral = sum of term (each times the radius
on the sphere), nseg = the count; both sums NaN where the length sum is 0 or the level is NaN; an infinite (or inf - inf) term
makes that level's integral NaN and leaves its length.
The periodic form is the same function on the plane with column 0 appended one period on (clength_periodic_ref.extend_plane),
the integrand extended with its own column 0.
"""
import numpy as np

import clength_ref as CR
import clength_periodic_ref as PR

RADIUS = CR.RADIUS


def point_values(F, r, c, nan_as=None):
    """F(u) of the end points (r, c) in index space: each lies on a grid row (r whole: a top / bottom point, between the columns
    floor(c) and floor(c) + 1) or on a grid column (c whole: a left / right point, between the rows floor(r) and floor(r) + 1);
    a point on a node takes the node's value either way.  `nan_as`: a deliberately wrong variant -- NaN nodes read as this"""
    F = np.asarray(F, dtype=np.float64)
    if nan_as is not None:
        F = np.where(np.isnan(F), nan_as, F)
    ny, nx = F.shape
    ri, ci = np.floor(r).astype(np.int64), np.floor(c).astype(np.int64)
    on_row = r == ri
    assert np.all(on_row | (c == ci))
    F0 = F[ri, ci]
    F1 = np.where(on_row, F[ri, np.minimum(ci + 1, nx - 1)], F[np.minimum(ri + 1, ny - 1), ci])
    t = np.where(on_row, c - ci, r - ri)
    with np.errstate(invalid='ignore', over='ignore'):
        return np.where(t == 0.0, F0, (F1 - F0) * t + F0)


def line_integrals(q2d, F2d, levels, ycoord, xcoord, latlon=False, weight=0.5, nan_as=None):
    """one slab -> (integral f64 (N,), length f64 (N,), nseg int64 (N,), sum |term| f64 (N,): the scale of the integral's
    rounding error, in the integral's units).  Levels in any order.  weight / nan_as: deliberately wrong variants for the tests
    of this restatement (the trapezoid weight; NaN nodes read as a number)"""
    lv = np.asarray(levels, dtype=np.float64)
    N = lv.size
    k, r1, c1, r2, c2, ln = CR.segments_fast(q2d, lv, ycoord, xcoord, latlon)
    Fu, Fv = point_values(F2d, r1, c1, nan_as), point_values(F2d, r2, c2, nan_as)
    keep = ~(np.isnan(Fu) | np.isnan(Fv))
    k, ln, Fu, Fv = k[keep], ln[keep], Fu[keep], Fv[keep]
    with np.errstate(invalid='ignore', over='ignore'):
        term = (weight * (Fu + Fv)) * ln
    nseg = np.bincount(k, minlength=N).astype(np.int64)
    length = np.bincount(k, weights=ln, minlength=N)
    bad = np.bincount(k, weights=(~np.isfinite(term)).astype(np.float64), minlength=N) > 0
    fin = np.where(np.isfinite(term), term, 0.0)
    integral = np.bincount(k, weights=fin, minlength=N)
    scale = np.bincount(k, weights=np.abs(fin), minlength=N)
    integral[bad] = np.nan
    none = (length == 0) | np.isnan(lv)
    if latlon:
        length, integral, scale = length * RADIUS, integral * RADIUS, scale * RADIUS
    length[none] = np.nan
    integral[none] = np.nan
    return integral, length, nseg, scale


def line_integrals_periodic(q2d, F2d, levels, ycoord, xcoord, period, latlon=False):
    qe, xe = PR.extend_plane(q2d, xcoord, period)
    Fe, _ = PR.extend_plane(F2d, xcoord, period)
    return line_integrals(qe, Fe, levels, ycoord, xe, latlon)


def stack(q, F, levels, ycoord, xcoord, latlon=False, period=None):
    """every slab of a stack -> the four arrays stacked (nslab, N); levels (N,) or (nslab, N)"""
    out = []
    for s in range(q.shape[0]):
        lv = levels[s] if np.ndim(levels) == 2 else levels
        out.append(line_integrals(q[s], F[s], lv, ycoord, xcoord, latlon) if period is None
                   else line_integrals_periodic(q[s], F[s], lv, ycoord, xcoord, period, latlon))
    return tuple(np.stack([o[i] for o in out]) for i in range(4))
