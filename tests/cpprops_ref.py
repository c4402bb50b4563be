"""K21 (xc_contour_piece_props_dev) restated on RAW RECORDS, from the header's definition (include/xcontour_hip.h, K21 section) -- a helper
for the tests, no tests here.  Input as for cptree_ref.piece_tree, on which it is built; `fields` a list of (ny, nx) or (nslab, ny, nx)
arrays (float32 ones are widened first), `w` None, (ny, nx) or (nslab, ny, nx), `x` (nslab, ny, nx) or None; range r reads slab r // ncont.

piece_props(): the SET rule, deliberately not the kernel's scan.  Per range the labels are cplabel_ref.labels_of_masks of
cptree_ref.piece_tree(..., return_masks=True).  A net sum is math.fsum of the float64 products w * g over label == p, a gross sum the same
over the ring's mask; NaN terms are skipped and an inf term gives NaN.  The extremum is taken over the nodes of label == p whose x is not
NaN, in the order of order_key (the usual monotone 64-bit key of a double: -0.0 below +0.0), ties to the smallest flat node r * nx + c;
NaN and -1 without such a node and for an open piece.  Returns (tables, props): per range cptree_ref's table and a dict of net, gross
(npiece, nf), x_min, x_max, at_min, at_max (None without x), rows in first_edge order.

scan_props(): what the kernels do instead, written out.  The state of every node is cplabel_ref.scan_labels' (the chunked scan with its
carries).  Every column is cut into the same chunks; a (chunk, column) walks its rows in scan order and gathers the terms and the keys
of the current state PRIVATELY; it hands them to the ring when the state changes and at the chunk's end; nodes in state -1 gather
nothing.  Then every ring adds what it gathered to itself and to every ancestor along parent[] (gross).  The places of the extrema
come from a second pass: the smallest flat node whose key equals the ring's.  Sums of the gathered terms are math.fsum (the kernel's
integer words are exact and free of order too).  `rows`: another chunk length.  `wrong`: one of WRONG -- a deliberately broken variant,
for the host tests that show the cases can tell:
  'no flush at the chunk end'       what a thread gathered is handed over at state changes only
  'fold reaches the parent only'    a ring's net terms reach its parent's gross sum and no further
  'tie takes the last node'         of equal keys the LARGEST flat node is taken
  'NaN wins the extremum'           a NaN is not skipped: it becomes both extrema of its ring
  'state -1 accumulates'            a node in no ring is added to row -1 of its range (the last row)"""
import math

import numpy as np

import cplabel_ref as LR
import cpinside_ref as PR
import cptree_ref as TR

WRONG = ('no flush at the chunk end', 'fold reaches the parent only', 'tie takes the last node', 'NaN wins the extremum',
         'state -1 accumulates')


def order_key(v):
    """the monotone uint64 key of float64 values, as Python ints"""
    b = int(np.float64(v).view(np.uint64))
    return (~b) & (2 ** 64 - 1) if b >> 63 else b | (1 << 63)


def exact_sum(terms, top=None):
    """math.fsum of the terms that are not NaN; NaN when one is infinite.  top: the terms are first cut in the window under 2^top
    (cinside_ref.window_sum)"""
    if top is not None:
        return TR.IR.window_sum(np.asarray(terms, dtype=np.float64), top)
    t = [float(v) for v in terms if v == v]
    return float('nan') if any(math.isinf(v) for v in t) else math.fsum(t)


def _planes(r, ncont, ny, nx, w, fields, x):
    """(the products w * g_m of range r's slab, each rounded once, float64 (ny, nx); x's plane or None)"""
    s = r // ncont
    wp = np.ones((ny, nx)) if w is None else np.asarray(w, dtype=np.float64)
    wp = wp[s] if wp.ndim == 3 else wp
    prods = []
    for g in fields:
        g = np.asarray(g)
        with np.errstate(all='ignore'):
            prods.append(wp * (g[s] if g.ndim == 3 else g).astype(np.float64))
    return prods, (None if x is None else np.asarray(x)[s].astype(np.float64))


def _extremum(xp, nodes, largest, wrong=None):
    """over the flat `nodes`: (value, flat node) of the smallest (largest) x that is not NaN, ties to the smallest node"""
    best = None
    for n in sorted(int(v) for v in nodes):
        v = xp.flat[n]
        if v != v:
            if wrong == 'NaN wins the extremum':
                return float('nan'), n
            continue
        k = order_key(v)
        k = -k if largest else k
        if best is None or k < best[0] or (k == best[0] and wrong == 'tie takes the last node'):
            best = (k, float(v), n)
    return (float('nan'), -1) if best is None else best[1:]


def _empty(n, nf, has_x):
    out = dict(net=np.full((n, nf), np.nan), gross=np.full((n, nf), np.nan))
    for k, t, v in (('x_min', np.float64, np.nan), ('x_max', np.float64, np.nan), ('at_min', np.int64, -1), ('at_max', np.int64, -1)):
        out[k] = np.full(n, v, dtype=t) if has_x else None
    return out


def field_tops(w, fields, nslab, ny, nx, bound=TR.IR.finite_bound):
    """-> per slab the list of the tops of the nf windows: field m's is cinside_ref.window_tops' top of w g_m -- the bound taken over the
    finite products of the slab's whole plane -- one window per (slab, field)"""
    per_field = [TR.IR.window_tops(w, np.broadcast_to(np.asarray(g), (nslab, ny, nx)), nslab, ny, nx, bound) for g in fields]
    return [[t[s][1] for t in per_field] for s in range(nslab)]


def piece_props(count, e_from, e_to, pts, ny, nx, periodic, flip=0, ncont=None, w=None, fields=(), x=None, tops=None):
    """tops: per slab the tops of the nf windows (field_tops) the net and gross sums are cut in; None: no term is cut (every term of the
    records suites lies wholly inside its window)"""
    tables, masks = TR.piece_tree(count, e_from, e_to, pts, ny, nx, periodic, flip=flip, ncont=ncont, w=w, return_masks=True)
    ncont = len(tables) if ncont is None else int(ncont)
    props = []
    for r, (t, ms) in enumerate(zip(tables, masks)):
        lab = LR.labels_of_masks(ms, (ny, nx))
        prods, xp = _planes(r, ncont, ny, nx, w, fields, x)
        out = _empty(t.size, len(fields), x is not None)
        for p, m in enumerate(ms):
            if m is None:
                continue
            for k, pr in enumerate(prods):
                top = None if tops is None else tops[r // ncont][k]
                out['net'][p, k], out['gross'][p, k] = exact_sum(pr[lab == p], top), exact_sum(pr[m], top)
            if xp is not None:
                nodes = np.flatnonzero(lab.ravel() == p)
                (out['x_min'][p], out['at_min'][p]), (out['x_max'][p], out['at_max'][p]) = _extremum(xp, nodes, False), _extremum(xp, nodes, True)
        props.append(out)
    return tables, props


def scan_props(count, e_from, e_to, pts, ny, nx, periodic, flip=0, ncont=None, w=None, fields=(), x=None, wrong=None, rows=None):
    """-> per range the dict of piece_props, by the kernels' route"""
    assert wrong is None or wrong in WRONG
    tables = TR.piece_tree(count, e_from, e_to, pts, ny, nx, periodic, flip=flip, ncont=ncont, w=w)
    states = LR.scan_labels(count, e_from, e_to, pts, ny, nx, periodic, flip=flip, rows=rows)
    ncont = len(tables) if ncont is None else int(ncont)
    R, nchunk = LR.scan_geometry(ny) if rows is None else (int(rows), -(-ny // int(rows)))
    nf, props = len(fields), []
    for r, (t, state) in enumerate(zip(tables, states)):
        prods, xp = _planes(r, ncont, ny, nx, w, fields, x)
        n = t.size
        terms = [[[] for _ in range(nf)] for _ in range(n)]                   # what reached the ring's staged words
        seen = [[] for _ in range(n)]                                        # the nodes whose key reached the ring
        for col in range(nx):
            for k in range(nchunk):
                cur, mine, nodes = None, [[] for _ in range(nf)], []

                def flush():
                    if cur is not None and cur >= 0 or (cur == -1 and wrong == 'state -1 accumulates' and n):
                        for m in range(nf):
                            terms[cur][m] += mine[m]
                        seen[cur].extend(nodes)
                for step in range(k * R, min((k + 1) * R, ny)):
                    at = ny - 1 - step if flip else step
                    s = int(state[at, col])
                    if s != cur:
                        flush()
                        cur, mine, nodes = s, [[] for _ in range(nf)], []
                    if s >= 0 or wrong == 'state -1 accumulates':
                        for m in range(nf):
                            mine[m].append(prods[m][at, col])
                        nodes.append(at * nx + col)
                if wrong != 'no flush at the chunk end':
                    flush()
        out = _empty(n, nf, x is not None)
        gross = [[list(terms[p][m]) for m in range(nf)] for p in range(n)]
        for p in range(n):                                                   # the fold: every ring adds its net terms to its ancestors
            q, steps = int(t['parent'][p]), 0
            while q >= 0 and t['closed'][p]:
                for m in range(nf):
                    gross[q][m] += terms[p][m]
                q, steps = (-1 if wrong == 'fold reaches the parent only' else int(t['parent'][q])), steps + 1
                assert steps <= n
        for p in range(n):
            if not t['closed'][p]:
                continue
            for m in range(nf):
                out['net'][p, m], out['gross'][p, m] = exact_sum(terms[p][m]), exact_sum(gross[p][m])
            if xp is not None:
                (out['x_min'][p], out['at_min'][p]) = _extremum(xp, seen[p], False, wrong)
                (out['x_max'][p], out['at_max'][p]) = _extremum(xp, seen[p], True, wrong)
        props.append(out)
    return props


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


def differences(got, ref):
    """the columns in which two props dicts differ: places equal, sums and extrema bit for bit (NaN in the same places; -0.0 is not +0.0)"""
    bad = [k for k in ('net', 'gross', 'x_min', 'x_max') if (got[k] is None) != (ref[k] is None) or (ref[k] is not None and not same_bits(got[k], ref[k]))]
    return bad + [k for k in ('at_min', 'at_max') if (got[k] is None) != (ref[k] is None) or (ref[k] is not None and not np.array_equal(got[k], ref[k]))]


# ------------------------------------------------------------------ the inputs the host and the GPU tests share
def field_set(rng, nf, nslab, ny, nx, scaled):
    """nf fields: float32 and float64 mixed, shared planes and per-slab stacks mixed (`scaled`: test_gpu_cpinside_records.scaled)"""
    return [scaled(rng, (nslab, ny, nx) if m % 3 != 1 else (ny, nx), np.float32 if m % 2 else np.float64) for m in range(nf)]


def integer_x(rng, nslab, ny, nx):
    """few integer values, a signed zero pair among them: ties, and -0.0 beside +0.0"""
    x = rng.integers(-2, 3, (nslab, ny, nx)).astype(np.float64)
    x[x == 0] = np.where(rng.random(int((x == 0).sum())) < 0.5, -0.0, 0.0)
    return x
