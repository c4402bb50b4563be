"""K17 (xc_contour_interior_dev) restated on RAW RECORDS, from the header's definition (include/xcontour_hip.h, K17 section) -- a
helper for the tests, no tests here.  Input: count[nrange], e_from, e_to, pts[total, 4], ny, nx, periodic, select -- what the C entry
takes -- and flip, ncont, w, f.

Pieces, per range: cpiece_records_ref.walk, as coverturn_ref takes them (contour_pieces_ref's rule on raw records).  Selection: K16's --
0 / 'all' every piece; 1 / 'circumpolar' every ring with winding != 0; 2 / 'main' the ring coverturn_ref.overturning names by
main_first_edge.  select != 0 on a plain plane raises ValueError.
X[r][c], 0 <= r < ny - 1: the vertical edge V(r, c) carries the start point of a selected piece's segment with odd e_from, or the end
point of an open piece's LAST segment in walk order with odd e_to; column (id >> 1) % nx, row (id >> 1) // nx (a row ny - 1 bounds no
node and is dropped).  P = the cumulative XOR of X down every column, P[0] = 0.  inside = P ^ flip.
Sums over the inside nodes of range s ncont + k: w (ones when None; (ny, nx) or (nslab, ny, nx)) and w * f[s] (one float64 product per
node, f cast to float64 first).  Each sum has a window of 160 bits under 2^top (window_tops: top = 12 + the frexp exponent of the largest
finite |w|, or |w f|, over ALL of the slab's plane, never below -800).  window_sum: NaN terms are dropped, any infinite term gives NaN,
else math.fsum of the terms cut toward zero at 2^(top - 160) -- zeros and denormals lie under every window.
scan_geometry(): the launch geometry of K17's scan restated, for the tests that must show which regime a shape lands in; it plays no part
in any expected value.
"""
import math

import numpy as np

import coverturn_ref as OR
import cpiece_records_ref as RR

SELECT = OR.SELECT


def crossing_flags(count, e_from, e_to, pts, ny, nx, periodic, select):
    """-> X uint8 (nrange, ny - 1, nx)"""
    sel = SELECT.get(select, select)
    assert sel in (0, 1, 2)
    if sel != 0 and not periodic:
        raise ValueError('select != 0 needs a periodic plane')
    count = np.asarray(count).astype(np.int64).ravel()
    ef, et = np.asarray(e_from, dtype=np.int64).ravel(), np.asarray(e_to, dtype=np.int64).ravel()
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 4)
    assert ef.size == et.size == pts.shape[0] == int(count.sum())
    main = OR.overturning(count, ef, et, pts, ny, nx, periodic, 0)['main_first_edge']
    X = np.zeros((count.size, max(ny - 1, 0), nx), dtype=np.uint8)
    s0 = 0
    for r, c in enumerate(count):
        sl = slice(s0, s0 + int(c))
        for segs, closed in RR.walk(ef[sl], et[sl], 2 * ny * nx):
            g = s0 + np.asarray(segs, dtype=np.int64)
            w = int((pts[g, 3] == nx).sum()) - int((pts[g, 1] == nx).sum()) if closed and periodic else 0
            chosen = sel == 0 or (w != 0 if sel == 1 else (w != 0 and int(ef[g].min()) == int(main[r])))
            if not chosen:
                continue
            ids = [int(ef[i]) for i in g if ef[i] & 1]
            if not closed and et[g[-1]] & 1:
                ids.append(int(et[g[-1]]))
            for e in ids:
                row, col = (e >> 1) // nx, (e >> 1) % nx
                if row < ny - 1:
                    X[r, row, col] = 1
        s0 += int(c)
    return X


def parity(X, ny):
    """P uint8 (nrange, ny, nx): the XOR of X over the rows above"""
    nr, _, nx = X.shape
    P = np.zeros((nr, ny, nx), dtype=np.uint8)
    if ny > 1:
        P[:, 1:] = np.bitwise_xor.accumulate(X, axis=1)
    return P


def nan_skipping_sum(terms):
    """plain math.fsum with K17's NaN and inf rules and NO window: what the sums are while every term lies wholly inside its window"""
    t = np.asarray(terms, dtype=np.float64).ravel()
    t = t[~np.isnan(t)]
    return float('nan') if np.isinf(t).any() else math.fsum(t.tolist())


def window_sum(terms, top):
    """the header's rule: NaN terms dropped; NaN if any term is infinite; else the exact sum, rounded once, of the terms with their bits
    under 2^(top - 160) cut off toward zero"""
    t = np.asarray(terms, dtype=np.float64).ravel()
    t = t[~np.isnan(t)]
    if np.isinf(t).any():
        return float('nan')
    return math.fsum(RR.cut(v, top - RR.WINDOW_BITS) for v in t.tolist())


def slab_planes(w, f, s, ny, nx):
    """-> (the float64 weights of slab s, its products w * float64(f[s]) or None): one product per node, rounded once"""
    wa = np.ones((ny, nx)) if w is None else np.asarray(w, dtype=np.float64)
    ws = wa[s] if wa.ndim == 3 else wa
    assert ws.shape == (ny, nx)
    if f is None:
        return ws, None
    with np.errstate(all='ignore'):
        return ws, ws * np.asarray(f[s]).astype(np.float64)


def finite_bound(v):
    """the largest |v| over the finite entries of v (0.0 when there is none)"""
    a = np.abs(np.asarray(v, dtype=np.float64).ravel())
    a = a[np.isfinite(a)]
    return float(a.max()) if a.size else 0.0


def window_tops(w, f, nslab, ny, nx, bound=finite_bound):
    """-> [(top_w, top_f)] per slab (top_f None without f): cpiece_records_ref.window_top of the largest |w| over the finite entries of
    the slab's plane (the shared plane, the slab's own with a 3-D w, 1.0 for w None) and of the largest |w * float64(f)| over the finite
    products -- all of the plane, inside or not.  `bound`: the host tests hand in broken rules."""
    tops = []
    for s in range(nslab):
        ws, wf = slab_planes(w, f, s, ny, nx)
        tops.append((RR.window_top(bound(ws)), None if wf is None else RR.window_top(bound(wf))))
    return tops


CI_TPB, CI_MIN_ROWS, CI_MAX_CHUNKS, CI_BLOCKS = 256, 4, 64, 4096            # the constants of xc_cinside.hip


def scan_geometry(ny, nx, nrange):
    """the scan's launch geometry as launch_contour_interior fixes it -> dict(ncb column blocks of 256, nchunk row chunks, rc rows per
    chunk, last = the rows of the last chunk, wpr 32-bit words per row of a bit plane)"""
    ncb = (nx + CI_TPB - 1) // CI_TPB
    nchunk = (CI_BLOCKS + ncb * nrange - 1) // (ncb * nrange)
    nchunk = min(nchunk, CI_MAX_CHUNKS, max(1, ny // CI_MIN_ROWS))
    rc = (ny + nchunk - 1) // nchunk
    nchunk = (ny + rc - 1) // rc
    return dict(ncb=ncb, nchunk=nchunk, rc=rc, last=ny - (nchunk - 1) * rc, wpr=(nx + 31) // 32)


def interior(count, e_from, e_to, pts, ny, nx, periodic, select, flip=0, ncont=None, w=None, f=None, tops=None):
    """-> dict(n_in int64 (nrange,), sum_w float64, sum_wf float64 or None, mask uint8 (nrange, ny, nx), X, tops [(top_w, top_f)] per
    slab).  `tops`: the windows to use instead of window_tops' (the host tests hand in those of broken bound rules)."""
    X = crossing_flags(count, e_from, e_to, pts, ny, nx, periodic, select)
    nr = X.shape[0]
    ncont = nr if ncont is None else int(ncont)
    assert nr % ncont == 0
    mask = parity(X, ny) ^ np.uint8(1 if flip else 0)
    if tops is None:
        tops = window_tops(w, f, nr // ncont, ny, nx)
    sum_w, sum_wf = np.empty(nr), (None if f is None else np.empty(nr))
    for r in range(nr):
        s = r // ncont
        ws, wf = slab_planes(w, f, s, ny, nx)
        inside = mask[r].astype(bool)
        sum_w[r] = window_sum(ws[inside], tops[s][0])
        if f is not None:
            sum_wf[r] = window_sum(wf[inside], tops[s][1])
    return dict(n_in=mask.reshape(nr, -1).sum(axis=1).astype(np.int64), sum_w=sum_w, sum_wf=sum_wf, mask=mask, X=X, tops=tops)


def same_bits(a, b):
    return OR.same_bits(a, b)
