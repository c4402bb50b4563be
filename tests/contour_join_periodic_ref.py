"""Restatement of K12 with a periodic X direction (xc_contour_segments_periodic) and of the lap / vertex / winding rule of
Contour2D.find_contours(periodic=...) -- a helper for the tests, no tests here.

Segments: contour_join_ref.segments on the plane with column 0 appended as column nx; every edge id folded from that
(ny, nx + 1) plane's numbering to the ring's -- (kind, r, c) -> 2 (r nx + (c mod nx)) + kind --; every range sorted by e_from
again.  The end points are untouched: columns in [0, nx], the seam cell's right edge at nx.

Polylines: contour_join_ref.join, then a plain loop.  In walk order a segment has the lap m: 0 for the first; between one
segment's end column and the next one's start column the jump is 0, +nx (m + 1) or -nx (m - 1).  Vertex columns: c + nx m in
index space, np.interp(c, arange(nx + 1), [x..., x[0] + P]) + m P in coordinates; the vertex rule is contour_join_ref's.
Winding of a ring: m_last + (c_end[last] - c_start[first]) / nx; of an open polyline 0.
"""
import numpy as np

import contour_join_ref as JR


def extend(q):
    """(..., ny, nx) -> (..., ny, nx + 1): column 0 appended as column nx"""
    q = np.asarray(q)
    return np.concatenate([q, q[..., :1]], axis=-1)


def fold_ids(e, nx):
    """edge ids of the (ny, nx + 1) plane -> the ring's"""
    e = np.asarray(e, dtype=np.int64)
    kind, cell = e & 1, e >> 1
    r, c = cell // (nx + 1), cell % (nx + 1)
    return 2 * (r * nx + c % nx) + kind


def fold_records(rec, nx):
    """records (count, e_from, e_to, pts) of a stack of extended planes, as Context.contour_segments or
    contour_join_ref.stack_records give them -> the ring's: ids folded, every range sorted by e_from again"""
    cnt, ef, et, pts = rec
    ef, et = fold_ids(ef, nx), fold_ids(et, nx)
    o = np.lexsort((ef, np.repeat(np.arange(cnt.size), cnt.ravel().astype(np.int64))))
    return cnt, ef[o], et[o], pts[o]


def segments(q2d, levels):
    """contour_join_ref.segments of the ring: per level (e_from, e_to, pts) sorted by e_from"""
    q = np.asarray(q2d, dtype=np.float64)
    nx = q.shape[1]
    assert nx >= 2
    out = []
    for ef, et, pts in JR.segments(extend(q), levels):
        ef, et = fold_ids(ef, nx), fold_ids(et, nx)
        o = np.argsort(ef, kind='stable')
        out.append((ef[o], et[o], pts[o]))
    return out


def stack_records(q, levels):
    """Context.contour_segments(q, levels, periodic=True) restated"""
    q = np.asarray(q)
    return fold_records(JR.stack_records(extend(q), levels), q.shape[-1])


def walk_polyline(pts, segs, ring, nx, ycoord=None, xcoord=None, period=None):
    """one joined polyline -> (vertices (n, 2) or None when fewer than two are left, winding, laps)"""
    laps, m = [0], 0
    for a, b in zip(segs[:-1], segs[1:]):
        jump = float(pts[a, 3]) - float(pts[b, 1])
        if jump == float(nx):
            m += 1
        elif jump == -float(nx):
            m -= 1
        else:
            assert jump == 0.0, jump
        laps.append(m)
    if ycoord is None:
        def vertex(r, c, m):
            return (float(r), float(c) + float(nx * m))
    else:
        yi, xi = np.arange(len(ycoord)), np.arange(nx + 1)
        y = np.asarray(ycoord, dtype=np.float64)
        xe = np.concatenate([np.asarray(xcoord, dtype=np.float64), [float(xcoord[0]) + float(period)]])

        def vertex(r, c, m):
            return (float(np.interp(r, yi, y)), float(np.interp(c, xi, xe)) + float(m) * float(period))
    v = [vertex(pts[segs[0], 0], pts[segs[0], 1], 0)] + [vertex(pts[i, 2], pts[i, 3], k) for i, k in zip(segs, laps)]
    merged = [v[0]]
    for p in v[1:]:
        if p != merged[-1]:
            merged.append(p)
    w = 0
    if ring:
        turn = (float(pts[segs[-1], 3]) - float(pts[segs[0], 1])) / float(nx)
        assert turn in (-1.0, 0.0, 1.0)
        w = laps[-1] + int(turn)
    return (np.array(merged, dtype=np.float64) if len(merged) >= 2 else None), w, laps


def polylines(q2d, levels, ycoord=None, xcoord=None, period=None):
    """Contour2D.find_contours(periodic=...) of one plane -> (out[k] lists of (n, 2) arrays, closed[k] lists of bools, winding[k]
    lists of ints); index space unless coordinates and the period are given"""
    nx = np.asarray(q2d).shape[1]
    out, closed, wind = [], [], []
    for ef, et, pts in segments(q2d, levels):
        ps, cl, ws = [], [], []
        for segs, ring in JR.join(ef, et):
            v, w, _ = walk_polyline(pts, segs, ring, nx, ycoord, xcoord, period)
            if v is not None:
                ps.append(v); cl.append(ring); ws.append(w)
        out.append(ps); closed.append(cl); wind.append(ws)
    return out, closed, wind


def census(q2d, levels, periodic=True):
    """per level [(number of segments, closed, winding), ...] of every joined polyline, dropped ones included; periodic=False:
    the plain plane (winding 0)"""
    nx = np.asarray(q2d).shape[1]
    out = []
    for ef, et, pts in (segments(q2d, levels) if periodic else JR.segments(q2d, levels)):
        row = []
        for segs, ring in JR.join(ef, et):
            row.append((len(segs), ring, walk_polyline(pts, segs, ring, nx)[1] if periodic else 0))
        out.append(row)
    return out
