"""A numpy restatement of K28 (xc_contour_distance_profile_dev: composites by distance) -- a helper, no tests here.

The distance of every node is cdist_ref.distance's (the restatement of K27), the sign cinside_ref's mask (the restatement of K17),
the cap cdist_ref's.  THE BIN RULE: a node with the final distance d belongs to bin b when edges[b] <= d < edges[b + 1]; d == edges[M]
belongs to bin M - 1 (np.histogram's rule); a node with d = +inf, or outside [edges[0], edges[M]], belongs nowhere.  That is
np.searchsorted(edges, d, 'right') - 1 with the last edge closed.  Per (range, bin): the nodes, the sum of w and the sums of w * f_m,
every product one float64 product, every sum math.fsum of its terms with K17's rules (a NaN term skipped, an infinite one gives NaN)."""
import numpy as np

import cdist_ref as DR
import cinside_ref as CI

RULES = ('histogram', 'last edge open', 'left open')


def bins_of(d, edges, rule='histogram'):
    """the bin of every distance, -1 for none.  rule: 'histogram' is the kernel's; the two others are deliberately wrong ones --
    'last edge open' leaves d == edges[M] out, 'left open' takes edges[b] < d <= edges[b + 1]"""
    e, d = np.asarray(edges, dtype=np.float64), np.asarray(d, dtype=np.float64)
    M = e.size - 1
    if rule == 'left open':
        b = np.searchsorted(e, d, 'left') - 1
    else:
        b = np.searchsorted(e, d, 'right') - 1
        if rule == 'histogram':
            b = np.where(d == e[M], M - 1, b)
    return np.where(np.isfinite(d) & (b >= 0) & (b < M), b, -1)


def profile(dist, edges, ncont, w=None, fields=(), rule='histogram'):
    """dist (nrange, ny, nx) as K27 stores it (+inf: no distance) -> dict(nodes int64 (nrange, M), area float64 (nrange, M), sums
    float64 (nf, nrange, M)); range r belongs to slab r // ncont; w: None, (ny, nx) or (nslab, ny, nx); a field (ny, nx) or
    (nslab, ny, nx), float32 or float64 (the product is taken in float64 from the cast value)"""
    dist = np.asarray(dist, dtype=np.float64)
    nrange, ny, nx = dist.shape
    M = len(edges) - 1
    out = dict(nodes=np.zeros((nrange, M), dtype=np.int64), area=np.zeros((nrange, M)), sums=np.zeros((len(fields), nrange, M)))
    for r in range(nrange):
        s = r // ncont
        b = bins_of(dist[r], edges, rule)
        wa = np.ones((ny, nx)) if w is None else np.asarray(w, dtype=np.float64)
        ws = wa[s] if wa.ndim == 3 else wa
        terms = [ws] + [ws * np.asarray(f[s] if np.ndim(f) == 3 else f).astype(np.float64) for f in fields]
        for k in range(M):
            at = b == k
            out['nodes'][r, k] = int(at.sum())
            out['area'][r, k] = CI.nan_skipping_sum(terms[0][at])
            for m in range(len(fields)):
                out['sums'][m, r, k] = CI.nan_skipping_sum(terms[1 + m][at])
    return out


def distances(rec, ny, nx, periodic, select, ycoord, xcoord, period=0.0, radius=0.0, max_dist=0.0, signed=False, flip=0):
    """the distance planes K28 bins: cdist_ref.distance with the cap, and with `signed` the sign of cinside_ref's mask"""
    mask = CI.interior(*rec, ny, nx, periodic, select, flip=flip)['mask'] if signed else None
    return DR.distance(*rec, ny, nx, periodic, select, ycoord, xcoord, period, radius, max_dist=max_dist, negate_mask=mask)['dist']


def reference(rec, ny, nx, periodic, select, ycoord, xcoord, edges, ncont, w=None, fields=(), period=0.0, radius=0.0, max_dist=0.0,
              signed=False, flip=0, rule='histogram'):
    d = distances(rec, ny, nx, periodic, select, ycoord, xcoord, period, radius, max_dist, signed, flip)
    return profile(d, edges, ncont, w, fields, rule)


def same_bits(a, b):
    return DR.same_bits(a, b)
