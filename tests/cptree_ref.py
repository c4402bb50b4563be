"""K19 (xc_contour_piece_tree_dev) restated on RAW RECORDS, from the header's definition (include/xcontour_hip.h, K19 section) -- a helper
for the tests, no tests here.  Input as for cpinside_ref.piece_interiors, on which it is built.

piece_tree(): brute force on sets, deliberately NOT the kernel's walk.  Per range the inside set of every ring is cpinside_ref's bool
mask.  a encloses b iff mask_b is a subset of mask_a (asserted on the way: two rings are nested or disjoint, and no two rings have the
same set); the parent is the enclosing ring of smallest cardinality; depth and nchild follow; the net set is the ring's mask minus its
children's masks; the net sums are cpinside_ref's sums (cinside_ref.window_sum: math.fsum of the terms in K18's window -- the slab's, or
the `tops` handed in -- each product rounded once, NaN terms dropped) over the net set, NaN exactly where the gross sum is NaN.  Open pieces: parent -1, depth 0, nchild 0,
n_net -1, NaN net sums.  Returns per range a structured array (DTYPE) sorted by first_edge, `parent` a row of that array."""
import numpy as np

import cinside_ref as IR
import cpinside_ref as PR

TREE_FIELDS = [('parent', np.int64), ('depth', np.int32), ('nchild', np.int32), ('n_net', np.int64), ('net_w', np.float64),
               ('net_wf', np.float64)]
DTYPE = np.dtype(PR.DTYPE.descr + TREE_FIELDS)
INT_FIELDS = PR.INT_FIELDS + ('parent', 'depth', 'nchild', 'n_net')
SUM_FIELDS = ('sum_w', 'sum_wf', 'net_w', 'net_wf')


def tree_of_masks(masks):
    """masks: per piece a bool (ny, nx) array, or None for an open piece -> (parent, depth, nchild) int64 arrays over the pieces"""
    n = len(masks)
    parent, depth, nchild = np.full(n, -1, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    rings = [k for k, m in enumerate(masks) if m is not None]
    if not rings:
        return parent, depth, nchild
    M = np.stack([masks[k].ravel() for k in rings]).astype(np.int64)
    size = M.sum(axis=1)
    common = M @ M.T
    for i in range(len(rings)):
        best = -1
        for j in range(len(rings)):
            if i == j:
                continue
            c = common[i, j]
            assert c == 0 or c == size[i] or c == size[j], 'two rings that are neither nested nor disjoint'
            assert not (c == size[i] == size[j]), 'two rings with the same inside set'
            if c == size[i] and (best < 0 or size[j] < size[best]):
                best = j
        if best >= 0:
            parent[rings[i]] = rings[best]
            nchild[rings[best]] += 1
    for k in rings:
        q, d = parent[k], 0
        while q >= 0:
            q, d = parent[q], d + 1
            assert d <= n
        depth[k] = d
    return parent, depth, nchild


def piece_tree(count, e_from, e_to, pts, ny, nx, periodic, flip=0, ncont=None, w=None, f=None, return_masks=False, tops=None):
    """-> per range a DTYPE array sorted by first_edge[, per range the list of inside masks in the same order].  `tops`: per slab the
    windows (top_w, top_f) to use instead of cinside_ref.window_tops' -- gross and net sums are cut in the same ones"""
    tables, masks, tops = PR.piece_interiors(count, e_from, e_to, pts, ny, nx, periodic, flip=flip, ncont=ncont, w=w, f=f,
                                             return_masks=True, return_tops=True, tops=tops)
    ncont = len(tables) if ncont is None else int(ncont)
    out = []
    for r, (t, ms) in enumerate(zip(tables, masks)):
        g = np.empty(t.size, dtype=DTYPE)
        for k in PR.DTYPE.names:
            g[k] = t[k]
        g['parent'], g['depth'], g['nchild'] = tree_of_masks(ms)
        for p, m in enumerate(ms):
            if m is None:
                g['n_net'][p], g['net_w'][p], g['net_wf'][p] = -1, np.nan, np.nan
                continue
            net = m.copy()
            for c in np.flatnonzero(g['parent'] == p):
                assert (ms[c] & ~m).sum() == 0
                net &= ~ms[c]
            sw, swf, _ = PR._sums(net, r, ncont, ny, nx, w, f, tops)
            g['n_net'][p] = int(net.sum())
            g['net_w'][p] = np.nan if np.isnan(t['sum_w'][p]) else sw
            g['net_wf'][p] = np.nan if np.isnan(t['sum_wf'][p]) else swf
        out.append(g)
    return (out, masks) if return_masks else out


def differences(got, ref):
    """the fields in which two tables (DTYPE arrays) differ: integers equal, the four sums bit for bit (NaN in the same places)"""
    if got.shape != ref.shape:
        return ['shape']
    bad = [k for k in INT_FIELDS if not np.array_equal(got[k], ref[k])]
    return bad + [k for k in SUM_FIELDS if not IR.same_bits(got[k], ref[k])]
