"""K20 (xc_contour_piece_labels_dev) restated on RAW RECORDS, from the header's definition (include/xcontour_hip.h, K20 section) -- a helper
for the tests, no tests here.  Input as for cptree_ref.piece_tree, on which it is built.

labels_of_masks(): the set rule, deliberately NOT the kernel's scan.  Per range the inside set of every ring is cpinside_ref's bool mask
(what cptree_ref.piece_tree(..., return_masks=True) returns, in first_edge order); a node's label is the ring whose mask holds it and
has the fewest nodes, -1 where no mask holds it.  Open pieces (None) never appear.

scan_labels(): what the kernel does instead, written out -- every column is scanned from the row that lies outside every ring (row 0, with
flip row ny - 1), in state -1; a crossing of a ring x has x's inside below it iff (s == S_x) != (winding_x != 0 and flip) (K18's s and S,
as in test_cptree_host.walk_parents); inside on the far side: the state becomes x; else it becomes parent[x] (the set rule's parent).  The
column is cut into the chunks of scan_geometry, as the launcher cuts it: per chunk but the last the state behind its last crossing of a
ring is carried (NONE without one), and a chunk starts from the nearest carry behind it that is not NONE, else from -1.  `rows`: another
chunk length than the launcher's.  `wrong`: one of WRONG -- a deliberately broken scan, for the host tests that show the cases can tell:
  'leave keeps the ring'    a crossing that leaves x leaves the state at x instead of taking x's parent
  'flip ignored'            the scan runs down from row 0 whatever flip is
  'open pieces are rings'   the crossings of an open piece enter and leave it like a ring's
Both return per range an int32 (ny, nx) array of rows of the range's first_edge-sorted table."""
import numpy as np

import cpinside_ref as PR
import cptree_ref as TR

WRONG = ('leave keeps the ring', 'flip ignored', 'open pieces are rings')
NONE = -2
PL_ROWS, PL_CHUNKS = 16, 32


def scan_geometry(ny):
    """the launch regime of the label scan: a column of ny rows is cut into `nchunk` chunks of `rows` rows (the last one what is left):
    at least PL_ROWS rows each, at most PL_CHUNKS chunks; with one chunk no carry pass runs -> (rows, nchunk)"""
    rows = max(PL_ROWS, -(-int(ny) // PL_CHUNKS))
    return rows, -(-int(ny) // rows)


def labels_of_masks(masks, shape=None):
    """masks: per piece of ONE range a bool (ny, nx) array, or None for an open piece -> int32 (ny, nx); `shape`: (ny, nx), needed where
    no piece is a ring"""
    rings = [k for k, m in enumerate(masks) if m is not None]
    shape = masks[rings[0]].shape if rings else tuple(shape)
    lab = np.full(shape, -1, dtype=np.int32)
    best = np.full(shape, np.iinfo(np.int64).max, dtype=np.int64)
    for k in rings:
        size = int(masks[k].sum())
        take = masks[k] & (size < best)
        assert not (masks[k] & (size == best)).any(), 'two rings with as many nodes round one node'
        lab[take], best[take] = k, size
    return lab


def scan_labels(count, e_from, e_to, pts, ny, nx, periodic, flip=0, wrong=None, rows=None):
    """-> per range the labels of the scan, int32 (ny, nx)"""
    assert wrong is None or wrong in WRONG
    count, ef, et, pts = PR._ranges(count, e_from, e_to, pts)
    trees = TR.piece_tree(count, ef, et, pts, ny, nx, periodic, flip=flip)
    R, nchunk = scan_geometry(ny) if rows is None else (int(rows), -(-ny // int(rows)))
    up = bool(flip) and wrong != 'flip ignored'
    out, s0 = [], 0
    for c, tree in zip(count, trees):
        pcs = sorted(PR._pieces(ef, et, pts, s0, c, ny, nx, periodic), key=lambda t: t[3])
        owner, sign, S, ring = {}, {}, [], []
        for k, (g, closed, wind, _) in enumerate(pcs):
            ring.append(closed or wrong == 'open pieces are rings')
            A = B = 0
            for i in g[(ef[g] & 1) == 1]:
                node = int(ef[i]) >> 1
                row, col = node // nx, node % nx
                if row >= ny - 1:
                    continue
                right = 2 * (row * nx + (col + 1) % nx) + 1
                s = 1 if int(et[i]) in (2 * node, 2 * (node + nx), right) else -1
                owner[(row, col)], sign[(row, col)] = k, s
                A, B = A + s, B + s * row
            S.append(((A > 0) - (A < 0)) if wind != 0 else ((B < 0) - (B > 0)))
        parent = tree['parent']

        def cross(e, col):
            x = owner.get((e, col))
            if x is None or not ring[x] or S[x] == 0:
                return NONE
            below = (sign[(e, col)] == S[x]) != (pcs[x][2] != 0 and bool(flip))
            if below != up:                                                   # the inside on the walker's far side
                return x
            return x if wrong == 'leave keeps the ring' else int(parent[x])

        lab = np.full((ny, nx), -7, dtype=np.int32)
        for col in range(nx):
            carry = [NONE] * nchunk
            for k in range(nchunk - 1):
                for t in range(k * R, min((k + 1) * R, ny - 1)):
                    v = cross(ny - 2 - t if up else t, col)
                    carry[k] = v if v != NONE else carry[k]
            for k in range(nchunk):
                state = next((carry[kk] for kk in range(k - 1, -1, -1) if carry[kk] != NONE), -1)
                for t in range(k * R, min((k + 1) * R, ny)):
                    at = ny - 1 - t if up else t
                    lab[at, col] = state
                    if t == ny - 1:
                        break
                    v = cross(at - 1 if up else at, col)
                    state = v if v != NONE else state
        assert (lab != -7).all()
        out.append(lab)
        s0 += int(c)
    return out
