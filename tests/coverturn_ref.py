"""K16 (xc_contour_overturning_dev) restated on RAW RECORDS, from the header's definition (include/xcontour_hip.h, K16 section) -- a
helper for the tests, no tests here.  Input: count[nrange], e_from, e_to, pts[total, 4], ny, nx, periodic, select -- what the C
entry takes.

Pieces, per range: cpiece_records_ref.walk (next(i) is the segment whose e_from == e_to[i]; the open pieces from their heads in
walk order, then the rings).  nseg, first_edge (the smallest e_from) and winding (#(c2 == nx) - #(c1 == nx) over a ring's segments
on a periodic plane, else 0) are K13's.
Selection: 0 / 'all' every piece; 1 / 'circumpolar' every ring with winding != 0; 2 / 'main' of those the one with the most segments,
ties broken by the smallest first_edge.  select != 0 on a plain plane raises ValueError.
Crossings of a selected piece: the start point of every segment whose e_from is odd, and the end point of an open piece's LAST
segment in walk order when its e_to is odd.  Column (id >> 1) % nx, row r1 / r2 of that record.
Output, a dict: ncross int32, row_lo / row_hi float64 (nrange, nx), NaN where ncross == 0; nsel int32, main_first_edge int64 (-1),
main_nseg int64 (0), main_winding int32 (0) (nrange,).

`wrong`: one of WRONG -- a deliberately broken rule, for the host tests that show the cases can tell:
  'e_to on rings'    the end point of EVERY segment with an odd e_to is counted too (a ring's vertices twice)
  'no selection'     every piece is counted whatever `select` says
  'first_edge only'  the main ring is the circumpolar ring of smallest first_edge, whatever its size
  'no fold'          the column is id >> 1 without the % nx (kept inside the row by a clip: rows past the first land on nx - 1)
"""
import numpy as np

import cpiece_records_ref as RR

SELECT = {'all': 0, 'circumpolar': 1, 'main': 2}
WRONG = ('e_to on rings', 'no selection', 'first_edge only', 'no fold')
INT_FIELDS = ('ncross', 'nsel', 'main_first_edge', 'main_nseg', 'main_winding')
FIELDS = ('ncross', 'row_lo', 'row_hi', 'nsel', 'main_first_edge', 'main_nseg', 'main_winding')


def overturning(count, e_from, e_to, pts, ny, nx, periodic, select, wrong=None):
    assert wrong is None or wrong in WRONG
    sel = SELECT.get(select, select)
    assert sel in (0, 1, 2)
    if sel != 0 and not periodic:
        raise ValueError('select != 0 needs a periodic plane')
    count = np.asarray(count).astype(np.int64).ravel()
    ef, et = np.asarray(e_from, dtype=np.int64).ravel(), np.asarray(e_to, dtype=np.int64).ravel()
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 4)
    assert ef.size == et.size == pts.shape[0] == int(count.sum())
    nr = count.size
    out = dict(ncross=np.zeros((nr, nx), dtype=np.int32), row_lo=np.full((nr, nx), np.nan), row_hi=np.full((nr, nx), np.nan),
               nsel=np.zeros(nr, dtype=np.int32), main_first_edge=np.full(nr, -1, dtype=np.int64), main_nseg=np.zeros(nr, dtype=np.int64),
               main_winding=np.zeros(nr, dtype=np.int32))
    s0 = 0
    for r, c in enumerate(count):
        sl = slice(s0, s0 + int(c))
        pieces = []
        for segs, closed in RR.walk(ef[sl], et[sl], 2 * ny * nx):
            g = s0 + np.asarray(segs, dtype=np.int64)
            w = int((pts[g, 3] == nx).sum()) - int((pts[g, 1] == nx).sum()) if closed and periodic else 0
            pieces.append(dict(g=g, closed=closed, nseg=int(g.size), first=int(ef[g].min()), w=w))
        circ = [p for p in pieces if p['closed'] and p['w'] != 0]
        main = None
        if circ:
            rank = (lambda p: (0, -p['first'])) if wrong == 'first_edge only' else (lambda p: (p['nseg'], -p['first']))
            main = max(circ, key=rank)
            out['main_first_edge'][r], out['main_nseg'][r], out['main_winding'][r] = main['first'], main['nseg'], main['w']
        chosen = pieces if sel == 0 else circ if sel == 1 else ([main] if main is not None else [])
        out['nsel'][r] = len(chosen)
        if wrong == 'no selection':
            chosen = pieces
        hits = []                                                            # (edge id, row)
        for p in chosen:
            g = p['g']
            hits += [(int(ef[i]), pts[i, 0]) for i in g if ef[i] & 1]
            ends = g if wrong == 'e_to on rings' else ([] if p['closed'] else g[-1:])
            hits += [(int(et[i]), pts[i, 2]) for i in ends if et[i] & 1]
        for e, row in hits:
            col = min(e >> 1, nx - 1) if wrong == 'no fold' else (e >> 1) % nx
            out['ncross'][r, col] += 1
            lo, hi = out['row_lo'][r, col], out['row_hi'][r, col]
            out['row_lo'][r, col] = row if np.isnan(lo) or row < lo else lo
            out['row_hi'][r, col] = row if np.isnan(hi) or row > hi else hi
        s0 += int(c)
    return out


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


def differences(got, ref):
    """the fields in which two results differ (integers equal, rows bit for bit, NaN in the same places) -> a list of names"""
    bad = []
    for f in FIELDS:
        a, b = np.asarray(got[f]), np.asarray(ref[f])
        if a.shape != b.shape or not (same_bits(a, b) if f in ('row_lo', 'row_hi') else (a.dtype == b.dtype and np.array_equal(a, b))):
            bad.append(f)
    return bad
