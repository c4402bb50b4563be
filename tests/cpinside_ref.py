"""K18 (xc_contour_piece_interiors_dev) restated on RAW RECORDS, from the header's definition (include/xcontour_hip.h, K18 section) -- a
helper for the tests, no tests here.  Input: count[nrange], e_from, e_to, pts[total, 4], ny, nx, periodic -- what the C entry takes --
and flip, ncont, w, f.

piece_interiors(): brute force, no orientation trick.  Pieces, per range: cpiece_records_ref.walk.  For ONE piece p: X_p[r][c] = 1 iff
V(r, c), r < ny - 1, carries the start point of a segment of p with odd e_from (or, on an open piece, the end point of its last segment
in walk order with odd e_to); P_p = cinside_ref.parity(X_p).  Ring of winding 0: inside = P_p; ring of winding != 0: inside = P_p ^ flip;
open piece: n_in = -1 and NaN sums.  Sums: cinside_ref.window_sum on the windows of cinside_ref.window_tops (NaN terms dropped, any
infinite term gives NaN, else math.fsum of the terms cut toward zero at the bottom of the slab's window).
Returns per range a structured array (DTYPE) sorted by first_edge (and the masks and the windows' tops when asked for).

mapping(): what the kernel does instead of scanning the plane once per piece, written out -- each crossing of a ring gets s = +1 when
its segment lies in the cell to the right of its vertical edge (e_to is that cell's top, bottom or right edge), else -1; per ring
A = sum s, B = sum s * row; S = sign(A) for winding != 0, else +1 for B < 0 and -1 for B > 0; a crossing with s == S walks down its column
from row r + 1 and stops behind the next crossing of its own piece or at row ny - 1 (winding != 0 with flip: up from row r, stopping
before the previous own crossing or at row 0).  `wrong`: one of WRONG -- a deliberately broken mapping, for the host tests that show the
cases can tell:
  'sign not per piece'       S = +1 for every ring
  'exit row included'        a walk takes one node more, the one behind the crossing it stops at
  'nested nodes subtracted'  a walk stops at the next crossing of ANY piece of the range
"""
import numpy as np

import cinside_ref as IR
import cpiece_records_ref as RR

DTYPE = np.dtype([('first_edge', np.int64), ('nseg', np.int64), ('closed', np.bool_), ('winding', np.int32),
                  ('n_in', np.int64), ('sum_w', np.float64), ('sum_wf', np.float64)])
INT_FIELDS = ('first_edge', 'nseg', 'closed', 'winding', 'n_in')
WRONG = ('sign not per piece', 'exit row included', 'nested nodes subtracted')


def _ranges(count, e_from, e_to, pts):
    count = np.asarray(count).astype(np.int64).ravel()
    ef, et = np.asarray(e_from, dtype=np.int64).ravel(), np.asarray(e_to, dtype=np.int64).ravel()
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 4)
    assert ef.size == et.size == pts.shape[0] == int(count.sum())
    return count, ef, et, pts


def _pieces(ef, et, pts, s0, c, ny, nx, periodic):
    """the pieces of one range -> [(global segment indices in walk order, closed, winding, first_edge)]"""
    out = []
    sl = slice(s0, s0 + int(c))
    for segs, closed in RR.walk(ef[sl], et[sl], 2 * ny * nx):
        g = s0 + np.asarray(segs, dtype=np.int64)
        w = int((pts[g, 3] == nx).sum()) - int((pts[g, 1] == nx).sum()) if closed and periodic else 0
        out.append((g, bool(closed), w, int(ef[g].min())))
    return out


def _sums(inside, r, ncont, ny, nx, w, f, tops):
    """-> (sum_w, sum_wf, (top_w, top_f)) of one piece of range r"""
    s = r // ncont
    ws, wf = IR.slab_planes(w, f, s, ny, nx)
    sw = IR.window_sum(ws[inside], tops[s][0])
    swf = np.nan if wf is None else IR.window_sum(wf[inside], tops[s][1])
    return sw, swf, tops[s]


def piece_interiors(count, e_from, e_to, pts, ny, nx, periodic, flip=0, ncont=None, w=None, f=None, return_masks=False,
                    return_tops=False, tops=None):
    """-> per range a DTYPE array sorted by first_edge[, per range the list of bool masks (ny, nx) in the same order; None for an open
    piece][, per slab the windows' tops (top_w, top_f)].  `tops`: the windows to use instead of cinside_ref.window_tops' (the host tests
    hand in those of broken bound rules)."""
    count, ef, et, pts = _ranges(count, e_from, e_to, pts)
    ncont = count.size if ncont is None else int(ncont)
    assert count.size % ncont == 0
    if tops is None:
        tops = IR.window_tops(w, f, count.size // ncont, ny, nx)
    tables, masks, s0 = [], [], 0
    for r, c in enumerate(count):
        rows = []
        for g, closed, wind, first in _pieces(ef, et, pts, s0, c, ny, nx, periodic):
            if not closed:
                rows.append(((first, g.size, False, 0, -1, np.nan, np.nan), None))
                continue
            X = np.zeros((1, max(ny - 1, 0), nx), dtype=np.uint8)
            for e in ef[g][(ef[g] & 1) == 1]:
                row, col = (int(e) >> 1) // nx, (int(e) >> 1) % nx
                if row < ny - 1:
                    X[0, row, col] = 1
            inside = (IR.parity(X, ny)[0] ^ np.uint8(1 if (flip and wind != 0) else 0)).astype(bool)
            sw, swf, _ = _sums(inside, r, ncont, ny, nx, w, f, tops)
            rows.append(((first, g.size, True, wind, int(inside.sum()), sw, swf), inside))
        rows.sort(key=lambda t: t[0][0])
        tables.append(np.array([t[0] for t in rows], dtype=DTYPE))
        masks.append([t[1] for t in rows])
        s0 += int(c)
    out = (tables,) + ((masks,) if return_masks else ()) + ((tops,) if return_tops else ())
    return out if len(out) > 1 else tables


def mapping(count, e_from, e_to, pts, ny, nx, periodic, flip=0, wrong=None):
    """the kernel's mapping -> per range the list of inside masks (bool (ny, nx); None for an open piece) in first_edge order"""
    assert wrong is None or wrong in WRONG
    count, ef, et, pts = _ranges(count, e_from, e_to, pts)
    out, s0 = [], 0
    for r, c in enumerate(count):
        pcs = _pieces(ef, et, pts, s0, c, ny, nx, periodic)
        owner = {}                                                           # (row, col) of a crossing -> the index of its piece
        for k, (g, closed, _, _) in enumerate(pcs):
            for e in ef[g][(ef[g] & 1) == 1]:
                owner[((int(e) >> 1) // nx, (int(e) >> 1) % nx)] = k
        rows = []
        for k, (g, closed, wind, first) in enumerate(pcs):
            if not closed:
                rows.append((first, None))
                continue
            cross = []
            for i in g[(ef[g] & 1) == 1]:
                node = int(ef[i]) >> 1
                row, col = node // nx, node % nx
                if row >= ny - 1:
                    continue
                right = 2 * (row * nx + (col + 1) % nx) + 1
                s = 1 if int(et[i]) in (2 * node, 2 * (node + nx), right) else -1
                cross.append((row, col, s))
            A, B = sum(s for _, _, s in cross), sum(s * row for row, _, s in cross)
            S = ((A > 0) - (A < 0)) if wind != 0 else ((B < 0) - (B > 0))
            if wrong == 'sign not per piece':
                S = 1
            up = wind != 0 and bool(flip)
            inside = np.zeros((ny, nx), dtype=bool)
            stops = (lambda key: key in owner) if wrong == 'nested nodes subtracted' else (lambda key: owner.get(key) == k)
            for row, col, s in cross:
                if S == 0 or s != S:
                    continue
                at = row if up else row + 1
                for _ in range(ny):
                    assert not inside[at, col], 'two walks met'
                    inside[at, col] = True
                    if at == (0 if up else ny - 1):
                        break
                    if stops((at - 1 if up else at, col)):
                        if wrong == 'exit row included':
                            inside[at + (-1 if up else 1), col] = True
                        break
                    at += -1 if up else 1
            rows.append((first, inside))
        rows.sort(key=lambda t: t[0])
        out.append([t[1] for t in rows])
        s0 += int(c)
    return out


def same_masks(a, b):
    """two results of mapping() / the masks of piece_interiors() alike?"""
    if len(a) != len(b):
        return False
    for ra, rb in zip(a, b):
        if len(ra) != len(rb):
            return False
        for ma, mb in zip(ra, rb):
            if (ma is None) != (mb is None) or (ma is not None and not np.array_equal(ma, mb)):
                return False
    return True


def differences(got, ref):
    """the fields in which two tables (DTYPE arrays) differ: integers equal, sums bit for bit (NaN in the same places)"""
    if got.shape != ref.shape:
        return ['shape']
    bad = [k for k in INT_FIELDS if not np.array_equal(got[k], ref[k])]
    return bad + [k for k in ('sum_w', 'sum_wf') if not IR.same_bits(got[k], ref[k])]
