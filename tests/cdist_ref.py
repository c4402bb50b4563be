"""K27 (xc_contour_distance_dev) restated on RAW RECORDS, from the header's definition (include/xcontour_hip.h, K27 section) -- a helper
for the tests, no tests here.  Brute force: every node against every selected segment, vectorised over the nodes, every operation a
numpy call of its own (rounded once, in the header's order), so the plane metric is the kernel's bit for bit.

Pieces and the selection are coverturn_ref's (cpiece_records_ref.walk, K16's tie rule); end points map to coordinates through
cpiece_records_ref.interp_nodes / x_nodes, as K13's do.  Segments are taken in ascending e_from with a strict `<`, so among equal
d2 / c2 the smallest id wins.  `nodes` = (rows, cols) restricts the nodes to a sub-grid (the outputs then have that shape).

`wrong`: one of WRONG -- a deliberately broken rule, for the host tests that show the cases can tell:
  'no clamp'     t is clamped at 0 only (the foot runs past b); on the sphere the arc test looks at a's side only
  'line'         the infinite line / the whole great circle instead of the segment
  'no shift'     no periodic images on the plane
  'tie larger'   among equal d2 / c2 the LARGEST id wins
pruned(): the tile / block walk of the kernel on the plane with the box-to-box bounds of xc_cdist_metric.h, or with
bound='centre' -- the distance of the box centres, which is no lower bound and prunes too much --, or with bound='gap skip ties'
-- the right bound under a skip rule that is not strict, which loses a tying block.  It counts the pairs it visits as the kernel
counts pairs_visited, and with nearest=True names the winner.
"""
import numpy as np

import cpiece_records_ref as RR

SELECT = {'all': 0, 'circumpolar': 1, 'main': 2}
WRONG = ('no clamp', 'line', 'no shift', 'tie larger')
RING = float(np.float64(np.deg2rad(np.float32(360.0))))
TILE, BLOCK = 16, 32
NODES_AT_ONCE = 1024


def selected(count, e_from, e_to, pts, ny, nx, periodic, select):
    """-> per range (indices of the selected segments into the packed records, ascending e_from; the first_edge of each one's piece)"""
    sel = SELECT.get(select, select)
    if sel != 0 and not periodic:
        raise ValueError('select != 0 needs a periodic plane')
    count = np.asarray(count).astype(np.int64).ravel()
    ef, et = np.asarray(e_from, dtype=np.int64).ravel(), np.asarray(e_to, dtype=np.int64).ravel()
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 4)
    out, s0 = [], 0
    for c in count:
        sl = slice(s0, s0 + int(c))
        pieces = []
        for segs, closed in RR.walk(ef[sl], et[sl], 2 * ny * nx):
            g = s0 + np.asarray(segs, dtype=np.int64)
            w = int((pts[g, 3] == nx).sum()) - int((pts[g, 1] == nx).sum()) if closed and periodic else 0
            pieces.append((g, closed and w != 0, int(g.size), int(ef[g].min())))
        circ = [p for p in pieces if p[1]]
        main = max(circ, key=lambda p: (p[2], -p[3])) if circ else None
        chosen = pieces if sel == 0 else circ if sel == 1 else ([main] if main is not None else [])
        idx = np.concatenate([p[0] for p in chosen]) if chosen else np.empty(0, dtype=np.int64)
        first = np.concatenate([np.full(p[2], p[3], dtype=np.int64) for p in chosen]) if chosen else np.empty(0, dtype=np.int64)
        o = np.argsort(ef[idx], kind='stable')
        out.append((idx[o], first[o]))
        s0 += int(c)
    return out


def end_points(pts, ny, nx, ycoord, xcoord, periodic, period):
    """-> (Y1, X1, Y2, X2) of every record, as K13 maps them"""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 4)
    y, xe = np.asarray(ycoord, dtype=np.float64), RR.x_nodes(xcoord, periodic, period)
    return RR.interp_nodes(pts[:, 0], y), RR.interp_nodes(pts[:, 1], xe), RR.interp_nodes(pts[:, 2], y), RR.interp_nodes(pts[:, 3], xe)


def d2_plane(py, px, ay, ax, by, bx, wrong=None):
    """nodes (n, 1) against segments (1, m) -> d2 (n, m), the header's operations one by one"""
    with np.errstate(all='ignore'):
        uy, ux = by - ay, bx - ax
        wy, wx = py - ay, px - ax
        uu = uy * uy + ux * ux
        t = (wy * uy + wx * ux) / uu
        if wrong == 'no clamp':
            t = np.maximum(t, 0.0)
        elif wrong != 'line':
            t = np.clip(t, 0.0, 1.0)
        t = np.where(uu == 0.0, 0.0, t)
        fy, fx = ay + t * uy, ax + t * ux
        dy, dx = py - fy, px - fx
        return dy * dy + dx * dx


def unit(y, x):
    c = np.cos(y)
    return np.stack([c * np.cos(x), c * np.sin(x), np.sin(y)], axis=-1)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _chord2(p, a):
    d = p - a
    return _dot(d, d)


def c2_sphere(p, a, b, wrong=None):
    """unit vectors p (n, 1, 3) against arcs a -> b (1, m, 3) -> the squared chord (n, m)"""
    with np.errstate(all='ignore'):
        n = _cross(a, b - a)
        nn = _dot(n, n)
        ca, cb = _chord2(p, a), _chord2(p, b)
        pn = _dot(p, n)
        s2 = (pn * pn) / nn
        arc = (2.0 * s2) / (1.0 + np.sqrt(1.0 - np.minimum(s2, 1.0)))
        on = _dot(_cross(a, p), n) >= 0.0
        if wrong != 'no clamp':
            on = on & (_dot(_cross(p, b), n) >= 0.0)
        if wrong == 'line':
            on = np.ones_like(on)
        return np.where(nn == 0.0, ca, np.where(on, arc, np.minimum(ca, cb)))


def best_of(D, ids, wrong=None):
    """D (n, m) over segments of ascending ids -> (min, id of the winner): the smallest id among equal values"""
    if D.shape[1] == 0:
        return np.full(D.shape[0], np.inf), np.full(D.shape[0], -1, dtype=np.int64), np.full(D.shape[0], -1, dtype=np.int64)
    D = np.where(np.isnan(D), np.inf, D)
    j = D.shape[1] - 1 - np.argmin(D[:, ::-1], axis=1) if wrong == 'tie larger' else np.argmin(D, axis=1)
    return D[np.arange(D.shape[0]), j], ids[j], j


def metric(py, px, Y1, X1, Y2, X2, periodic, period, radius, wrong=None, chunk=256):
    """nodes (n,) against segments (m,) of ascending ids 0 .. m-1 -> (min d2 / c2 (n,), the winner's position (n,), -1 without one)"""
    n, m = py.size, Y1.size
    if n > NODES_AT_ONCE:                                    # (element-wise throughout: slabs of nodes that stay in the cache give the same bits)
        parts = [metric(py[i:i + NODES_AT_ONCE], px[i:i + NODES_AT_ONCE], Y1, X1, Y2, X2, periodic, period, radius, wrong, chunk)
                 for i in range(0, n, NODES_AT_ONCE)]
        return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    best, at = np.full(n, np.inf), np.full(n, -1, dtype=np.int64)
    if radius > 0.0:
        P = unit(py, px)[:, None, :]
    for c0 in range(0, m, chunk):
        sl = slice(c0, min(m, c0 + chunk))
        if radius > 0.0:
            D = c2_sphere(P, unit(Y1[sl], X1[sl])[None], unit(Y2[sl], X2[sl])[None], wrong)
        else:
            seg = (Y1[None, sl], X1[None, sl], Y2[None, sl], X2[None, sl])
            D = d2_plane(py[:, None], px[:, None], *seg, wrong=wrong)
            if periodic and wrong != 'no shift':
                D = np.fmin(D, d2_plane(py[:, None], (px + period)[:, None], *seg, wrong=wrong))
                D = np.fmin(D, d2_plane(py[:, None], (px - period)[:, None], *seg, wrong=wrong))
        d, _, j = best_of(D, np.arange(sl.start, sl.stop), wrong)
        take = (d <= best) & (j >= 0) & np.isfinite(d) if wrong == 'tie larger' else d < best
        best, at = np.where(take, d, best), np.where(take, c0 + j, at)
    return best, at


def finish(best, radius):
    """min d2 / c2 -> the distance"""
    with np.errstate(all='ignore'):
        if radius > 0.0:
            return radius * (2.0 * np.arcsin(np.minimum(1.0, np.sqrt(best) * 0.5)))
        return np.sqrt(best)


def distance(count, e_from, e_to, pts, ny, nx, periodic, select, ycoord, xcoord, period=0.0, radius=0.0, max_dist=0.0,
             negate_mask=None, wrong=None, nodes=None, winners=None):
    """-> dict(dist float64, edge, piece int64 (nrange, rows, cols), best: the winning d2 / c2, at: the winner's place among the
    range's selected segments).  winners: the result of an earlier call on the same records, select, nodes and rule -- its best and
    at are taken over and only the cap and the mask, which come after the search, are applied anew."""
    ef = np.asarray(e_from, dtype=np.int64).ravel()
    ycoord, xcoord = np.asarray(ycoord, dtype=np.float64), np.asarray(xcoord, dtype=np.float64)
    period = np.float64(period if periodic else 0.0)
    rows, cols = (np.arange(ny), np.arange(nx)) if nodes is None else nodes
    PY, PX = [v.ravel() for v in np.meshgrid(ycoord[rows], xcoord[cols], indexing='ij')]
    Y1, X1, Y2, X2 = end_points(pts, ny, nx, ycoord, xcoord, periodic, period)
    sel = selected(count, e_from, e_to, pts, ny, nx, periodic, select)
    shape = (len(sel), rows.size, cols.size)
    out = dict(dist=np.full(shape, np.inf), edge=np.full(shape, -1, dtype=np.int64), piece=np.full(shape, -1, dtype=np.int64),
               best=np.full(shape, np.inf), at=np.full(shape, -1, dtype=np.int64))
    for r, (idx, first) in enumerate(sel):
        if winners is not None:
            best, at = winners['best'][r].ravel(), winners['at'][r].ravel()
        else:
            best, at = metric(PY, PX, Y1[idx], X1[idx], Y2[idx], X2[idx], periodic, period, radius, wrong)
        d = finish(best, radius)
        has = at >= 0
        if max_dist > 0.0 and np.isfinite(max_dist):
            has &= ~(d > max_dist)
        d = np.where(has, d, np.inf)
        if negate_mask is not None:
            m = np.asarray(negate_mask).reshape(len(sel), ny, nx)[r][np.ix_(rows, cols)].ravel() != 0
            d = np.where(m & has, -d, d)
        out['dist'][r] = d.reshape(shape[1:])
        out['best'][r] = best.reshape(shape[1:])
        out['at'][r] = at.reshape(shape[1:])
        out['edge'][r] = np.where(has, ef[idx][np.maximum(at, 0)] if idx.size else -1, -1).reshape(shape[1:])
        out['piece'][r] = np.where(has, first[np.maximum(at, 0)] if idx.size else -1, -1).reshape(shape[1:])
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((a.view(np.int64) == b.view(np.int64)).all())


def pruned(e_from, pts, ny, nx, ycoord, xcoord, periodic=False, period=0.0, bound='gap', nearest=False):
    """The kernel's walk on the plane for ONE range with every segment selected: tiles of TILE x TILE nodes, blocks of BLOCK x BLOCK
    cells by the cell of e_from, in ascending block order, a block's box the hull of a and fl(a + fl(b - a)); a tile takes W = the
    smallest far distance to a block, then every block whose bound does not exceed min(W, its worst best-distance so far).
    -> (min d2 (ny, nx), pairs visited), with `nearest` -> (min d2, pairs visited, the winner's id (ny, nx), its position in the
    records as given (ny, nx)): among equal d2 the smallest id, as best_of; -1 without a winner.
    bound 'gap': the box-to-box gap, a block skipped only where it EXCEEDS W; 'gap skip ties': the same gap, a block skipped where it
    reaches W (a tying block is lost); 'centre': the distance of the box centres (no lower bound)."""
    ef = np.asarray(e_from, dtype=np.int64).ravel()
    ycoord, xcoord = np.asarray(ycoord, dtype=np.float64), np.asarray(xcoord, dtype=np.float64)
    period = np.float64(period if periodic else 0.0)
    Y1, X1, Y2, X2 = end_points(pts, ny, nx, ycoord, xcoord, periodic, period)
    o = np.argsort(ef, kind='stable')
    ef, Y1, X1, Y2, X2 = ef[o], Y1[o], X1[o], Y2[o], X2[o]
    node = ef >> 1
    bid = (node // nx // BLOCK) * ((nx + BLOCK - 1) // BLOCK) + (node % nx) // BLOCK
    blocks = []
    for b in np.unique(bid):
        g = np.flatnonzero(bid == b)
        ey, ex = Y1[g] + (Y2[g] - Y1[g]), X1[g] + (X2[g] - X1[g])
        blocks.append((g, min(Y1[g].min(), ey.min()), max(Y1[g].max(), ey.max()), min(X1[g].min(), ex.min()), max(X1[g].max(), ex.max())))
    shifts = (0.0, period, -period) if periodic else (0.0,)
    gap = lambda tlo, thi, blo, bhi: max(0.0, tlo - bhi, blo - thi)
    far = lambda tlo, thi, blo, bhi: max(thi - blo, bhi - tlo)
    out, pairs = np.full((ny, nx), np.inf), 0
    edge, pos = np.full((ny, nx), -1, dtype=np.int64), np.full((ny, nx), -1, dtype=np.int64)
    for r0 in range(0, ny, TILE):
        for c0 in range(0, nx, TILE):
            rows, cols = np.arange(r0, min(ny, r0 + TILE)), np.arange(c0, min(nx, c0 + TILE))
            PY, PX = [v.ravel() for v in np.meshgrid(ycoord[rows], xcoord[cols], indexing='ij')]
            tyl, tyh = PY.min(), PY.max()
            tx = [((PX + s).min(), (PX + s).max()) for s in shifts]

            def lower(b):
                if bound == 'centre':
                    cy, cx = 0.5 * (tyl + tyh) - 0.5 * (b[1] + b[2]), 0.5 * (tx[0][0] + tx[0][1]) - 0.5 * (b[3] + b[4])
                    return cy * cy + cx * cx
                gy = gap(tyl, tyh, b[1], b[2])
                return min(gy * gy + gap(lo, hi, b[3], b[4]) ** 2 for lo, hi in tx)
            W = min(min(far(tyl, tyh, b[1], b[2]) ** 2 + far(lo, hi, b[3], b[4]) ** 2 for lo, hi in tx) for b in blocks) if blocks else np.inf
            best, at = np.full(PY.size, np.inf), np.full(PY.size, -1, dtype=np.int64)
            for b in blocks:
                lb = lower(b)
                if lb >= W if bound == 'gap skip ties' else lb > W:
                    continue
                g = b[0]
                d, j = metric(PY, PX, Y1[g], X1[g], Y2[g], X2[g], periodic, period, 0.0)
                take = (j >= 0) & ((d < best) | ((d == best) & (g[np.maximum(j, 0)] < at)))       # (positions ascend with the ids)
                best, at = np.where(take, d, best), np.where(take, g[np.maximum(j, 0)], at)
                pairs += PY.size * g.size
                W = min(W, best.max())
            out[np.ix_(rows, cols)] = best.reshape(rows.size, cols.size)
            if not blocks:
                continue
            has = at >= 0
            edge[np.ix_(rows, cols)] = np.where(has, ef[np.maximum(at, 0)], -1).reshape(rows.size, cols.size)
            pos[np.ix_(rows, cols)] = np.where(has, o[np.maximum(at, 0)], -1).reshape(rows.size, cols.size)
    return (out, pairs, edge, pos) if nearest else (out, pairs)
