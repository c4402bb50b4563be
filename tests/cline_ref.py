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
    F0, F1, t = edge_nodes(F, r, c)
    with np.errstate(invalid='ignore', over='ignore'):
        return np.where(t == 0.0, F0, (F1 - F0) * t + F0)


def edge_nodes(F, r, c):
    """the edges that carry the end points (r, c): -> (F0, F1, t): the integrand on the edge's first and second node and the
    point's fraction along it (0: on the first node)"""
    F = np.asarray(F, dtype=np.float64)
    ny, nx = F.shape
    ri, ci = np.floor(r).astype(np.int64), np.floor(c).astype(np.int64)
    on_row = r == ri
    assert np.all(on_row | (c == ci))
    F0 = F[ri, ci]
    F1 = np.where(on_row, F[ri, np.minimum(ci + 1, nx - 1)], F[np.minimum(ri + 1, ny - 1), ci])
    return F0, F1, np.where(on_row, c - ci, r - ri)


def terms(q2d, F2d, levels, ycoord, xcoord, latlon=False, weight=0.5, nan_as=None):
    """the counted segments of one slab -> (k level index, len, term), NaN end-point values skipped"""
    lv = np.asarray(levels, dtype=np.float64)
    k, r1, c1, r2, c2, ln = CR.segments_fast(q2d, lv, ycoord, xcoord, latlon)
    Fu, Fv = point_values(F2d, r1, c1, nan_as), point_values(F2d, r2, c2, nan_as)
    keep = ~(np.isnan(Fu) | np.isnan(Fv))
    k, ln, Fu, Fv = k[keep], ln[keep], Fu[keep], Fv[keep]
    with np.errstate(invalid='ignore', over='ignore'):
        return k, ln, (weight * (Fu + Fv)) * ln


def line_integrals(q2d, F2d, levels, ycoord, xcoord, latlon=False, weight=0.5, nan_as=None):
    """one slab -> (integral f64 (N,), length f64 (N,), nseg int64 (N,), sum |term| f64 (N,): the scale of the integral's
    rounding error, in the integral's units).  Levels in any order.  weight / nan_as: deliberately wrong variants for the tests
    of this restatement (the trapezoid weight; NaN nodes read as a number)"""
    lv = np.asarray(levels, dtype=np.float64)
    N = lv.size
    k, ln, term = terms(q2d, F2d, lv, ycoord, xcoord, latlon, weight, nan_as)
    nseg = np.bincount(k, minlength=N).astype(np.int64)
    length = np.bincount(k, weights=ln, minlength=N).astype(np.float64)          # (no segment at all: bincount gives integers)
    bad = np.bincount(k, weights=(~np.isfinite(term)).astype(np.float64), minlength=N) > 0
    fin = np.where(np.isfinite(term), term, 0.0)
    integral = np.bincount(k, weights=fin, minlength=N).astype(np.float64)
    scale = np.bincount(k, weights=np.abs(fin), minlength=N).astype(np.float64)
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


# ---- K15's two fixed-point sums, modelled (the counterpart of clength_ref.det_totals)
def term_window_top(F2d, bound, f_dtype=np.float64, wrong=None):
    """the first bit of channel 1's window (k_cline_window): det_window_top((bound * m) * 1.0000001), m = max(|min F|, |max F|) over the
    slab's FINITE values after the cast to f_dtype, each product rounded once; a slab without a finite value: bound 0.
    wrong: 'max_f' -- m = max F --, 'nonfinite' -- the extrema over every value: deliberately wrong variants"""
    import xcontour_oracle as O
    F = np.asarray(F2d).astype(f_dtype).astype(np.float64)
    fin = F.ravel() if wrong == 'nonfinite' else F[np.isfinite(F)]
    if fin.size == 0:
        return O.det_window_top(0.0)
    with np.errstate(over='ignore', invalid='ignore'):
        m = float(np.max(fin)) if wrong == 'max_f' else max(abs(float(np.min(fin))), abs(float(np.max(fin))))
        return O.det_window_top(np.float64(np.float64(bound) * np.float64(m)) * np.float64(1.0000001))


def floor_chunk_sums(idx, w, nb, top, nlimb=4):
    """a deliberately wrong deterministic_bin_sums: the chunks of a NEGATIVE weight cut toward minus infinity (an arithmetic shift of
    the two's complement value), not toward zero -- both the 49-bit cut and the low chunk under the window"""
    import math
    from fractions import Fraction
    import xcontour_oracle as O
    out = np.zeros(nb)
    tot = [0] * nb
    ebot = top - O.DET_LIMB_BITS * nlimb
    for b, v in zip(np.asarray(idx) - 1, np.asarray(w, dtype=np.float64)):
        if v == 0 or not np.isfinite(v):
            continue
        m, e = math.frexp(float(v))
        n = int(math.floor(Fraction(m) * 2 ** O.DET_PREC_BITS))           # 49 bits, floor
        tot[b] += int(math.floor(Fraction(n) * Fraction(2) ** (e - O.DET_PREC_BITS - ebot)))
    for k in range(nb):
        out[k] = math.ldexp(float(tot[k]), ebot) if tot[k] else 0.0
    return out


def det_integrals(q2d, F2d, levels, ycoord, xcoord, latlon=False, period=None, f_dtype=np.float64, wrong=None):
    """K15's two sums, modelled, for one slab -> (integral f64 (N,), length f64 (N,)).  Levels ascending.
    The segments and terms are line_integrals' own (NaN end-point values skipped; the integrand cast to f_dtype first, as the
    kernel reads it).  Channel 0: the lengths through the oracle's fixed-point rule (deterministic_bin_sums, 4 limbs) on the window of
    clen_bound, as det_totals.  Channel 1: the terms, signed, through the same rule on the window of term_window_top; a non-finite
    term makes its level NaN.  Both NaN where the length sum is 0; each times the radius once on the sphere.  period: the periodic
    form, on the extended plane.
    wrong: deliberately wrong variants for the tests of this model -- 'floor' (floor_chunk_sums), 'max_f' and 'nonfinite'
    (term_window_top), 'len_window' (channel 1 summed on channel 0's window)"""
    import xcontour_oracle as O
    F = np.asarray(F2d).astype(f_dtype).astype(np.float64)
    if period is not None:
        F, _ = PR.extend_plane(F, xcoord, period)
        q2d, xcoord = PR.extend_plane(q2d, xcoord, period)
    lv = np.asarray(levels, dtype=np.float64)
    N = lv.size
    k, ln, term = terms(q2d, F, lv, ycoord, xcoord, latlon)
    bound = CR.clen_bound(ycoord, xcoord, latlon)
    top0 = O.det_window_top(bound)
    top1 = top0 if wrong == 'len_window' else term_window_top(F, bound, wrong=wrong if wrong in ('max_f', 'nonfinite') else None)
    length = O.deterministic_bin_sums(k + 1, ln, N, top=top0, nlimb=4)
    if wrong == 'floor':
        integral = floor_chunk_sums(k + 1, term, N, top1)
    else:
        integral = O.deterministic_bin_sums(k + 1, term, N, top=top1, nlimb=4)
    none = length == 0
    if latlon:
        length, integral = length * RADIUS, integral * RADIUS
    length[none] = np.nan
    integral[none] = np.nan
    return integral, length


# ---- inputs on which every term is three correctly rounded operations on exact inputs (the bit-for-bit rows)
FP_PROFILES = ('mixed', 'cancel', 'wide', 'under')


def fixed_point_case(profile, along_x, f_dtype=np.float64, ny=97, nx=301):
    """The planes of K10's test_fixed_point_rule_bit_for_bit -- spacings of 20 significant bits, a tracer that varies along one axis
    only (along_x: along x), some flat sides, the second slab the first turned round -- with an integrand that varies only ALONG the
    segments: along y where the tracer varies along x.  Every segment lies on a grid line, its length is one spacing exactly, and both
    nodes of every edge that carries an end point hold the same integrand value, so F(u) is a node value whatever the fraction.
    One node per slab, on the line of flat tracer that no segment touches (`lone`), may hold anything.  Profiles g (one value per
    node along the segments):
      'mixed'   signs mixed, magnitudes spread over 2^-30 .. 2^30; lone -inf (slab 0) and NaN (slab 1): outside the finite extrema
      'cancel'  two nodes of +B and -B', their neighbours 0, with B (d[a-1] + d[a]) == B' (d[b-1] + d[b]) exactly (B ~ 2^51): four
                terms of ~2^50 that cancel exactly; the rest ~0.01: the residue lies more than 2^40 below sum |term|
      'wide'    magnitudes ~2^-30, signs mixed; lone -2^120: the window bottom is ~2^-59 and every term drops its low chunk
      'under'   'mixed' magnitudes; lone 1e200: every term lies under the window, the integral is exactly 0
    -> q (2, ny, nx) f64, F (2, ny, nx) f_dtype, levels (33,), y, x"""
    y, x = CR.few_bits(ny, 1, 1.0), CR.few_bits(nx, 2, 1.0)
    rng = np.random.default_rng(len(profile) + 2 * int(along_x))
    prof = np.sort(rng.uniform(-3.0, 3.0, nx if along_x else ny))
    prof[::17] = prof[1::17][:prof[::17].size]
    plane = np.broadcast_to(prof[None, :] if along_x else prof[:, None], (ny, nx))
    q = np.stack([plane, plane[::-1, ::-1]]).astype(np.float64)
    lv = np.concatenate([np.sort(rng.uniform(-3.2, 3.2, 30)), prof[[5, 40, 77]]])
    lv.sort()
    n, d = (ny, np.diff(y)) if along_x else (nx, np.diff(x))          # nodes and spacings along the segments
    F = np.empty((2, ny, nx))
    for s in range(2):
        sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
        if profile in ('mixed', 'under'):
            g = sign * 2.0 ** rng.uniform(-30.0, 30.0, n) * rng.uniform(1.0, 2.0, n)
        elif profile == 'wide':
            g = sign * 2.0 ** -30 * rng.uniform(0.5, 2.0, n)
        else:
            g = 0.01 * rng.standard_normal(n)
            a, b = (20, 60) if s == 0 else (33, 71)
            g[a - 1:a + 2] = 0.0; g[b - 1:b + 2] = 0.0
            g[a] = 2.0 ** 50 * (d[b - 1] + d[b]); g[b] = -2.0 ** 50 * (d[a - 1] + d[a])
        g = g.astype(f_dtype).astype(np.float64)
        F[s] = np.broadcast_to(g[:, None] if along_x else g[None, :], (ny, nx))
        lone = {'mixed': (-np.inf, np.nan)[s], 'wide': -2.0 ** 120, 'under': 1e200}.get(profile)
        if lone is not None:                                          # the flat line: nodes 0 and 1 of prof are equal
            at = (0, -1)[s]
            F[(s, n // 2, at) if along_x else (s, at, n // 2)] = lone
    return q, F.astype(f_dtype), lv, y, x


def check_fixed_point_premise(q2d, F2d, lv, y, x):
    """the premise of the bit-for-bit rows, on the CPU: every length is one spacing exactly, and both nodes of every edge that carries
    an end point hold the same, finite, integrand value (or the point lies on the first node).  -> the number of segments"""
    k, r1, c1, r2, c2, ln = CR.segments_fast(q2d, lv, y, x)
    spac = np.concatenate([np.diff(y), np.diff(x)])
    assert k.size > 0 and np.isin(ln, spac).all()
    for r, c in ((r1, c1), (r2, c2)):
        F0, F1, t = edge_nodes(F2d, r, c)
        assert ((F0 == F1) | (t == 0.0)).all() and np.isfinite(F0).all()     # (t == 0: on the first node, the second does not enter)
    return k.size
