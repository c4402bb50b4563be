"""K24 (xc_contour_folds_dev) restated on RAW RECORDS, from the header's definition (include/xcontour_hip.h, K24 section) -- a helper
for the tests, no tests here.  Input: count[nrange], e_from, e_to, pts[total, 4], ny, nx, periodic, select -- what the C entry takes --
and gap, ncont, w, f.

X and P: cinside_ref's (K17's crossing flags and node parity under the same select).  For a column c of a range: n[c] = sum_r X[r][c],
lo[c] / hi[c] the smallest / largest r with X[r][c] = 1.  Folded: n[c] >= 3.  Fold nodes: (r, c), lo[c] < r <= hi[c]; tongue
t = P[r][c] ^ P[lo[c] + 1][c] (0 under, 1 over).  Event: a maximal set of folded columns with at most `gap` unfolded columns between
consecutive ones; on a periodic plane column nx - 1 is followed by column 0, and a range whose every cyclic gap is <= gap is one event
from its smallest folded column.  Events ordered by c_west; dx(c) = (c - c_west) mod nx.
row_lo / row_hi: coverturn_ref's (K16's) rows, NaN where n[c] == 0.
Sums per (event, tongue), math.fsum under cinside_ref.window_sum's rules (NaN terms dropped, an infinite term gives NaN, bits under
2^(top - 160) cut off): area = sum w, mx = sum w * dx, my = sum w * r, integral = sum w * float64(f) -- one float64 product per node.
tops(): top = cpiece_records_ref.window_top of max |w|, max |w| * nx, max |w| * ny (a product that overflows: the largest double),
max |w f| over the finite values of the slab's plane.

`wrong`: one of WRONG -- a deliberately broken rule, for the host tests that show the cases can tell:
  'n >= 2'                    a column with two crossings counts as folded
  'no seam join'              the run at column 0 of a periodic plane is never joined to the run at column nx - 1
  'gap ignored'               gap = 0 whatever was given
  'bridged columns labelled'  col_event names the event on the unfolded columns inside it too
  'tongue from P alone'       t = P[r][c]
  'dx without mod'            dx = c - c_west
  'hi excluded'               the fold nodes are lo < r < hi
"""
import sys

import numpy as np

import cinside_ref as IR
import coverturn_ref as OR
import cpiece_records_ref as RR

WRONG = ('n >= 2', 'no seam join', 'gap ignored', 'bridged columns labelled', 'tongue from P alone', 'dx without mod', 'hi excluded')
COL_FIELDS = ('ncross', 'row_lo', 'row_hi', 'col_event')
INT_FIELDS = ('c_west', 'c_east', 'ncol', 'ncross_max', 'nodes')
ROW_FIELDS = ('ev_row_lo', 'ev_row_hi')
SUM_FIELDS = ('area', 'mx', 'my', 'integral')


def runs(fold, gap, periodic, wrong=None):
    """the folded flags of one range -> the events, each the list of its folded columns going east from c_west, ordered by c_west"""
    nx = fold.size
    cols = np.flatnonzero(fold).tolist()
    if not cols:
        return []
    g = 0 if wrong == 'gap ignored' else gap
    out = [[cols[0]]]
    for a, b in zip(cols[:-1], cols[1:]):
        if b - a - 1 <= g:
            out[-1].append(b)
        else:
            out.append([b])
    if periodic and wrong != 'no seam join' and len(out) >= 2 and cols[0] + nx - cols[-1] - 1 <= g:
        out = out[1:-1] + [out[-1] + out[0]]
    return out


def tops(w, f, nslab, ny, nx):
    """-> [(area, mx, my, integral or None)] per slab"""
    big = sys.float_info.max
    out = []
    for s in range(nslab):
        ws, wf = IR.slab_planes(w, f, s, ny, nx)
        b = IR.finite_bound(ws)
        with np.errstate(over='ignore'):
            bx, by = min(float(np.float64(b) * np.float64(nx)), big), min(float(np.float64(b) * np.float64(ny)), big)
        out.append((RR.window_top(b), RR.window_top(bx), RR.window_top(by), None if wf is None else RR.window_top(IR.finite_bound(wf))))
    return out


def folds(count, e_from, e_to, pts, ny, nx, periodic, select, gap=0, ncont=None, w=None, f=None, wrong=None):
    """-> dict(ncross int32, row_lo, row_hi float64, col_event int32 (nrange, nx); event_count int64 (nrange,); per event, packed by
    range: c_west, c_east, ncol, ncross_max int32, ev_row_lo, ev_row_hi float64, nodes int64 (ne, 2), area, mx, my, integral float64
    (ne, 2) -- integral None without f)"""
    assert wrong is None or wrong in WRONG
    assert 0 <= gap < nx
    X = IR.crossing_flags(count, e_from, e_to, pts, ny, nx, periodic, select).astype(np.int64)
    P = IR.parity(X.astype(np.uint8), ny)
    k16 = OR.overturning(count, e_from, e_to, pts, ny, nx, periodic, select)
    nr = X.shape[0]
    ncont = nr if ncont is None else int(ncont)
    assert nr % ncont == 0
    n = X.sum(axis=1).astype(np.int32)
    row_lo, row_hi = np.where(n > 0, k16['row_lo'], np.nan), np.where(n > 0, k16['row_hi'], np.nan)
    col_event = np.full((nr, nx), -1, dtype=np.int32)
    T = tops(w, f, nr // ncont, ny, nx)
    ev = {k: [] for k in INT_FIELDS + ROW_FIELDS + SUM_FIELDS}
    event_count = np.zeros(nr, dtype=np.int64)
    for r in range(nr):
        s = r // ncont
        ws, wf = IR.slab_planes(w, f, s, ny, nx)
        fold = n[r] >= (2 if wrong == 'n >= 2' else 3)
        events = runs(fold, gap, periodic, wrong)
        event_count[r] = len(events)
        for j, cols in enumerate(events):
            cw, ce = cols[0], cols[-1]
            col_event[r, cols] = j
            if wrong == 'bridged columns labelled':
                c = cw
                while c != ce:
                    col_event[r, c] = j
                    c = (c + 1) % nx
            terms = {k: ([], []) for k in SUM_FIELDS}
            nodes = [0, 0]
            for c in cols:
                rows = np.flatnonzero(X[r, :, c])
                lo, hi = int(rows[0]), int(rows[-1])
                dx = float(c - cw if wrong == 'dx without mod' else (c - cw) % nx)
                for row in range(lo + 1, hi if wrong == 'hi excluded' else hi + 1):
                    t = int(P[r, row, c]) if wrong == 'tongue from P alone' else int(P[r, row, c] ^ P[r, lo + 1, c])
                    a = np.float64(ws[row, c])
                    nodes[t] += 1
                    with np.errstate(all='ignore'):
                        terms['area'][t].append(a)
                        terms['mx'][t].append(a * np.float64(dx))
                        terms['my'][t].append(a * np.float64(row))
                        if wf is not None:
                            terms['integral'][t].append(wf[row, c])
            ev['c_west'].append(cw); ev['c_east'].append(ce); ev['ncol'].append(len(cols)); ev['ncross_max'].append(int(n[r, cols].max()))
            ev['ev_row_lo'].append(row_lo[r, cols].min()); ev['ev_row_hi'].append(row_hi[r, cols].max())
            ev['nodes'].append(nodes)
            for i, k in enumerate(SUM_FIELDS):
                if k != 'integral' or wf is not None:
                    ev[k].append([IR.window_sum(terms[k][t], T[s][i]) for t in (0, 1)])
    ne = int(event_count.sum())
    out = dict(ncross=n, row_lo=row_lo, row_hi=row_hi, col_event=col_event, event_count=event_count, tops=T)
    for k in ('c_west', 'c_east', 'ncol', 'ncross_max'):
        out[k] = np.asarray(ev[k], dtype=np.int32).reshape(ne)
    out['nodes'] = np.asarray(ev['nodes'], dtype=np.int64).reshape(ne, 2)
    for k in ROW_FIELDS:
        out[k] = np.asarray(ev[k], dtype=np.float64).reshape(ne)
    for k in SUM_FIELDS:
        out[k] = None if (k == 'integral' and f is None) else np.asarray(ev[k], dtype=np.float64).reshape(ne, 2)
    return out


def same_bits(a, b):
    return OR.same_bits(a, b)


def differences(got, ref, events=True):
    """the fields in which two results differ (integers equal, floats bit for bit, NaN in the same places) -> a list of names"""
    bad = []
    names = COL_FIELDS + ('event_count',) + ((INT_FIELDS + ROW_FIELDS + SUM_FIELDS) if events else ())
    for k in names:
        a, b = got[k], ref[k]
        if a is None or b is None:
            if (a is None) != (b is None):
                bad.append(k)
            continue
        a, b = np.asarray(a), np.asarray(b)
        if a.shape != b.shape:
            bad.append(k)
        elif a.dtype.kind == 'f' or b.dtype.kind == 'f':
            if not same_bits(a, b):
                bad.append(k)
        elif not np.array_equal(a.astype(np.int64), b.astype(np.int64)):
            bad.append(k)
    return bad


# ------------------------------------------------------------------ hand-built planes: q = far ? 1 : 0, level 0.5
def plane(ny, nx, base):
    """rows >= base are far (1): one ring round a periodic plane, no fold"""
    m = np.zeros((ny, nx), dtype=np.uint8)
    m[base:] = 1
    return m


def hook(m, cols, stem, top, bottom, base):
    """a tongue of the far side over the columns `cols`, rows [top, bottom), joined to the far side through column `stem` (rows top ..
    base - 1): every column of `cols` gains two crossings, the stem column none.  bottom < base."""
    assert top < bottom < base
    m[top:bottom, list(cols)] = 1
    m[top:base, stem] = 1
    return m


def field(m):
    return m.astype(np.float64)


LEVEL = np.array([0.5])


def cases():
    """the hand-built planes of the suites: name -> (mask, periodic, select, gap)"""
    C = {}
    C['no fold'] = (plane(9, 8, 5), 1, 2, 0)
    C['hook of 3'] = (hook(plane(9, 8, 6), (3, 4), 5, 2, 4, 6), 1, 2, 0)
    five = hook(hook(plane(10, 8, 7), (3, 4), 5, 1, 2, 7), (3, 4), 5, 3, 5, 7)
    C['hook of 5'] = (five, 1, 2, 0)
    two = hook(hook(plane(9, 12, 6), (2, 3), 1, 2, 4, 6), (5, 6), 7, 1, 3, 6)
    for g in (0, 1, 2):
        C['two hooks, gap %d' % g] = (two, 1, 2, g)
    seam = hook(plane(9, 8, 6), (7, 0), 1, 2, 4, 6)
    C['seam hook, ring'] = (seam, 1, 2, 0)
    C['seam hook, plain'] = (seam, 0, 0, 0)
    band = plane(9, 8, 6)
    band[2:4] = 1
    C['every column folded'] = (band, 1, 0, 0)
    C['every column folded, gap 3'] = (band, 1, 0, 3)
    blob = plane(9, 8, 6)
    blob[2:4, 3:5] = 1
    C['blob, all'] = (blob, 1, 0, 0)
    C['blob, main'] = (blob, 1, 2, 0)
    lone = np.zeros((9, 8), dtype=np.uint8)
    lone[2:4, 3:5] = 1
    C['two crossings'] = (lone, 0, 0, 0)
    C['nx 33'] = (hook(plane(9, 33, 6), (31, 32), 30, 2, 4, 6), 1, 2, 0)
    C['nx 65'] = (hook(hook(plane(9, 65, 6), (63, 64), 62, 2, 4, 6), (30, 31, 32, 33), 34, 1, 3, 6), 1, 2, 0)
    C['nx 257'] = (hook(hook(plane(9, 257, 6), (254, 255, 256, 0, 1), 2, 2, 4, 6), tuple(range(60, 70)), 70, 1, 3, 6), 1, 2, 0)
    C['ny 300'] = (hook(plane(300, 8, 200), (3, 4), 5, 50, 120, 200), 1, 2, 0)
    return C
