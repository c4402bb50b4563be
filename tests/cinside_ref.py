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
node, f cast to float64 first).  NaN terms are dropped, any infinite term gives NaN, else math.fsum.
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
    t = np.asarray(terms, dtype=np.float64).ravel()
    t = t[~np.isnan(t)]
    return float('nan') if np.isinf(t).any() else math.fsum(t.tolist())


def interior(count, e_from, e_to, pts, ny, nx, periodic, select, flip=0, ncont=None, w=None, f=None):
    """-> dict(n_in int64 (nrange,), sum_w float64, sum_wf float64 or None, mask uint8 (nrange, ny, nx), X)"""
    X = crossing_flags(count, e_from, e_to, pts, ny, nx, periodic, select)
    nr = X.shape[0]
    ncont = nr if ncont is None else int(ncont)
    assert nr % ncont == 0
    mask = parity(X, ny) ^ np.uint8(1 if flip else 0)
    wa = np.ones((ny, nx)) if w is None else np.asarray(w, dtype=np.float64)
    sum_w, sum_wf = np.empty(nr), (None if f is None else np.empty(nr))
    for r in range(nr):
        s = r // ncont
        ws = wa[s] if wa.ndim == 3 else wa
        inside = mask[r].astype(bool)
        sum_w[r] = nan_skipping_sum(ws[inside])
        if f is not None:
            with np.errstate(all='ignore'):
                sum_wf[r] = nan_skipping_sum(ws[inside] * np.asarray(f[s], dtype=np.float64)[inside])
    return dict(n_in=mask.reshape(nr, -1).sum(axis=1).astype(np.int64), sum_w=sum_w, sum_wf=sum_wf, mask=mask, X=X)


def same_bits(a, b):
    return OR.same_bits(a, b)
