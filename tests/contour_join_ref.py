"""numpy / pure-Python restatement of K12 (xc_cseg.hip: directed contour segments with grid-edge ids), of the join rule of
xc_join_segments (xc_join.cpp) and of the vertex rule of Contour2D.find_contours -- a helper for the tests, no tests here.

Emission: the rule of clength_ref (the case table PAIRS, frac, NaN cells), every segment directed start -> end as PAIRS lists
it, saddles 6 -> (R, T), (L, B) and 9 -> (T, L), (B, R); a segment whose two end points coincide is KEPT.  Edge ids: the
horizontal edge between nodes (r, c) and (r, c+1) is 2 (r nx + c), the vertical edge between (r, c) and (r+1, c) is
2 (r nx + c) + 1; cell (r0, c0) has T = H(r0, c0), B = H(r0+1, c0), L = V(r0, c0), R = V(r0, c0+1).

Join, per level: next(i) is the segment whose e_from == e_to[i], prev(i) the one whose e_to == e_from[i] (dicts keyed by edge
id); a segment without prev heads an open polyline; every remaining segment lies on a ring, which starts at its segment of
smallest e_from; polylines are ordered by the smallest e_from they contain.

Vertices: start(s0), end(s0), end(s1), ...; consecutive equal vertices merged; polylines with fewer than two vertices dropped.
"""
import numpy as np

from clength_ref import PAIRS, T, B, L, R, _frac


def segments(q2d, levels):
    """every directed segment of every level of one plane -> per level k (in the order given; a NaN level has none) a tuple
    (e_from int64, e_to int64, pts float64 (n, 4) = r1, c1, r2, c2), sorted by e_from"""
    q = np.asarray(q2d, dtype=np.float64)
    lv = np.asarray(levels, dtype=np.float64)
    ny, nx = q.shape
    empty = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros((0, 4)))
    if ny < 2 or nx < 2:
        return [empty for _ in lv]
    ul, ur, ll, lr = q[:-1, :-1], q[:-1, 1:], q[1:, :-1], q[1:, 1:]
    ok = ~(np.isnan(ul) | np.isnan(ur) | np.isnan(ll) | np.isnan(lr))
    r0a, c0a = np.nonzero(ok)
    A, Bv, D, E = ul[ok], ur[ok], ll[ok], lr[ok]
    mn = np.fmin(np.fmin(A, Bv), np.fmin(D, E))
    mx = np.fmax(np.fmax(A, Bv), np.fmax(D, E))
    out = []
    for c in lv:
        if np.isnan(c):
            out.append(empty)
            continue
        sel = (mn <= c) & (c < mx)
        r0, c0 = r0a[sel].astype(np.int64), c0a[sel].astype(np.int64)
        a, b, d, e = A[sel], Bv[sel], D[sel], E[sel]
        case = (a > c) * 1 + (b > c) * 2 + (d > c) * 4 + (e > c) * 8
        r0f, c0f = r0.astype(np.float64), c0.astype(np.float64)
        pts = {T: (r0f, c0f + _frac(a, b, c)), B: (r0f + 1.0, c0f + _frac(d, e, c)),
               L: (r0f + _frac(a, d, c), c0f), R: (r0f + _frac(b, e, c), c0f + 1.0)}
        h = 2 * (r0 * nx + c0)
        eid = {T: h, B: h + 2 * nx, L: h + 1, R: h + 3}
        ef, et, pp = [], [], []
        for cs, prs in PAIRS.items():
            m = case == cs
            if not m.any():
                continue
            for p, s in prs:
                ef.append(eid[p][m]); et.append(eid[s][m])
                pp.append(np.stack([pts[p][0][m], pts[p][1][m], pts[s][0][m], pts[s][1][m]], axis=1))
        if not ef:
            out.append(empty)
            continue
        ef, et, pp = np.concatenate(ef), np.concatenate(et), np.concatenate(pp)
        o = np.argsort(ef, kind='stable')
        out.append((ef[o], et[o], pp[o]))
    return out


def stack_records(q, levels):
    """the records of a stack as Context.contour_segments returns them: (count (nslab, N) uint64, e_from, e_to, pts), packed by
    (slab, level), each range sorted by e_from.  levels (N,) or (nslab, N)."""
    q = np.asarray(q)
    lv = np.asarray(levels, dtype=np.float64)
    N = lv.shape[-1]
    cnt = np.zeros((q.shape[0], N), dtype=np.uint64)
    ef, et, pp = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)], [np.zeros((0, 4))]
    for s in range(q.shape[0]):
        for k, (a, b, p) in enumerate(segments(q[s], lv[s] if lv.ndim == 2 else lv)):
            cnt[s, k] = a.size
            ef.append(a); et.append(b); pp.append(p)
    return cnt, np.concatenate(ef), np.concatenate(et), np.concatenate(pp)


def join(e_from, e_to):
    """one range -> [(segment indices in walk order, closed), ...] ordered by the smallest e_from a polyline contains.
    Duplicate ids raise ValueError."""
    e_from, e_to = [int(v) for v in e_from], [int(v) for v in e_to]
    n = len(e_from)
    by_from = {e: i for i, e in enumerate(e_from)}
    by_to = {e: i for i, e in enumerate(e_to)}
    if len(by_from) != n or len(by_to) != n:
        raise ValueError('duplicate edge id')
    seen = [False] * n
    polys = []

    def walk(h):
        segs, i = [], h
        while i is not None and not seen[i]:
            seen[i] = True
            segs.append(i)
            i = by_from.get(e_to[i])
        return segs
    for i in range(n):
        if e_from[i] not in by_to:
            polys.append((walk(i), False))
    for i in sorted(range(n), key=lambda j: e_from[j]):
        if not seen[i]:
            polys.append((walk(i), True))
    polys.sort(key=lambda p: min(e_from[i] for i in p[0]))
    return polys


def vertices(pts, segs):
    """the vertex rule: start of the first segment, the end of every segment, consecutive equal vertices merged -> (n, 2), or
    None when fewer than two vertices are left"""
    v = [tuple(pts[segs[0], :2])] + [tuple(pts[i, 2:]) for i in segs]
    m = [v[0]]
    for p in v[1:]:
        if p != m[-1]:
            m.append(p)
    return np.array(m, dtype=np.float64) if len(m) >= 2 else None


def polylines(q2d, levels, ycoord=None, xcoord=None):
    """Contour2D.find_contours of one plane -> (out[k] = list of (n, 2) arrays, closed[k] = list of bools); index space unless
    coordinates are given (np.interp(., arange(n), coord) in float64)"""
    out, closed = [], []
    for ef, et, pts in segments(q2d, levels):
        if ycoord is not None and pts.size:
            yi, xi = np.arange(len(ycoord)), np.arange(len(xcoord))
            y, x = np.asarray(ycoord, dtype=np.float64), np.asarray(xcoord, dtype=np.float64)
            pts = np.stack([np.interp(pts[:, 0], yi, y), np.interp(pts[:, 1], xi, x),
                            np.interp(pts[:, 2], yi, y), np.interp(pts[:, 3], xi, x)], axis=1)
        ps, cl = [], []
        for segs, ring in join(ef, et):
            v = vertices(pts, segs)
            if v is not None:
                ps.append(v); cl.append(ring)
        out.append(ps); closed.append(cl)
    return out, closed
