"""Restatements of K22 (xc_label_overlap_dev) in numpy, for one range: two int32 maps (ny, nx), a weight plane w (None: 1) and an
integrand plane f (None: none) -> the rows (a, b, n, sum_w, sum_wf) sorted by (a, b).

overlap_of_maps   the SET rule: np.unique over the stacked pairs, math.fsum of the selected float64 terms.
scan_of_maps      the kernel's run walk: every column is cut into chunks of `chunk` rows, a walker keeps the current pair down its chunk
                  and hands a run over to a dict when the pair changes and at the chunk's end.
`broken` names a deliberate defect of the walk (test_cpoverlap_host.py shows that the cases catch each of them)."""
import math

import numpy as np

import cinside_ref as IR

DTYPE = np.dtype([('a', np.int32), ('b', np.int32), ('n', np.int64), ('sum_w', np.float64), ('sum_wf', np.float64)])


def terms(w, f, shape):
    """the float64 terms of the two sums: w (1 where None), and w * f with f widened first and the product rounded once (None where f is)"""
    tw = np.ones(shape) if w is None else np.asarray(w, dtype=np.float64)
    with np.errstate(all='ignore'):
        tf = None if f is None else tw * np.asarray(f).astype(np.float64)
    return tw, tf


def exact(v, top=None):
    """K17's sum of the terms v: NaN terms skipped, an infinite term gives NaN, else the exact sum rounded once -- of the terms as they are
    (top None: every term lies wholly inside its window), or of the terms cut in the window under 2^top (cinside_ref.window_sum)"""
    if top is not None:
        return IR.window_sum(v, top)
    v = v[~np.isnan(v)]
    return math.nan if np.isinf(v).any() else math.fsum(v.tolist())


def rows_of(table, tops=None):
    """{(a, b): (n, [terms of w], [terms of w f] or None)} -> the sorted rows.  tops: (top_w, top_f) of the range's slab"""
    top_w, top_f = (None, None) if tops is None else tops
    out = np.empty(len(table), dtype=DTYPE)
    for i, (a, b) in enumerate(sorted(table)):
        n, tw, tf = table[(a, b)]
        out[i] = (a, b, n, exact(np.asarray(tw, dtype=np.float64), top_w),
                  math.nan if tf is None else exact(np.asarray(tf, dtype=np.float64), top_f))
    return out


def overlap_of_maps(la, lb, w=None, f=None, tops=None):
    """tops: the windows (top_w, top_f) of the range's slab -- cinside_ref.window_tops of the slab's WHOLE plane, the nodes of the omitted
    pair (-1, -1) included; None: no term is cut (every existing case keeps its terms wholly inside the window)"""
    la, lb = np.asarray(la), np.asarray(lb)
    a = np.where(la < 0, -1, la).astype(np.int64).ravel()
    b = np.where(lb < 0, -1, lb).astype(np.int64).ravel()
    tw, tf = terms(w, f, la.shape)
    tw, tf = tw.ravel(), None if tf is None else tf.ravel()
    pairs, inv = np.unique(np.stack([a, b], axis=1), axis=0, return_inverse=True)
    inv = inv.ravel()
    table = {}
    for i, (pa, pb) in enumerate(pairs.tolist()):
        if pa == -1 and pb == -1:
            continue
        at = np.flatnonzero(inv == i)
        table[(pa, pb)] = (at.size, tw[at], None if tf is None else tf[at])
    return rows_of(table, tops)


def scan_of_maps(la, lb, w=None, f=None, chunk=16, broken=None):
    la, lb = np.asarray(la), np.asarray(lb)
    ny, nx = la.shape
    tw, tf = terms(w, f, la.shape)
    table = {}

    def norm(v):
        v = int(v)
        if broken == 'negative labels kept':
            return v
        return -1 if v < 0 else v

    def hand_over(pair, run):
        if pair is None or not run:
            return
        if broken == 'one-sided rows dropped' and pair[0] == -1:
            return
        key = (min(pair), max(pair)) if broken == 'unordered key' else pair
        n, sw, sf = table.setdefault(key, (0, [], None if tf is None else []))
        table[key] = (n + len(run), sw + [tw[r, c] for r, c in run], None if tf is None else sf + [tf[r, c] for r, c in run])

    for c in range(nx):
        for r0 in range(0, ny, chunk):
            cur, run = None, []
            for r in range(r0, min(r0 + chunk, ny)):
                pair = (norm(la[r, c]), norm(lb[r, c]))
                if pair == (-1, -1):
                    pair = None                                              # the empty key: nothing is gathered
                if pair != cur:
                    hand_over(cur, run)
                    cur, run = pair, []
                if pair is not None:
                    run.append((r, c))
            if broken != 'no flush at the chunk\'s end':
                hand_over(cur, run)
    return rows_of(table)


def count_runs(la, lb, chunk):
    """the runs of constant pair, other than (-1, -1), down the chunks: the kernel's bound on the distinct pairs"""
    la, lb = np.where(np.asarray(la) < 0, -1, la), np.where(np.asarray(lb) < 0, -1, lb)
    ny = la.shape[0]
    runs = 0
    for r0 in range(0, ny, chunk):
        a, b = la[r0:r0 + chunk], lb[r0:r0 + chunk]
        full = ~((a == -1) & (b == -1))
        start = np.ones_like(full)
        start[1:] = (a[1:] != a[:-1]) | (b[1:] != b[:-1])
        runs += int((full & start).sum())
    return runs


def same(got, ref):
    """rows equal: integers equal, sums bit for bit (NaN = NaN)"""
    def bits(v):
        v = np.array(v, dtype=np.float64)
        v[np.isnan(v)] = np.nan                                              # one NaN
        return v.view(np.uint64)
    return (got.size == ref.size and all(np.array_equal(got[k], ref[k]) for k in ('a', 'b', 'n'))
            and all(np.array_equal(bits(got[k]), bits(ref[k])) for k in ('sum_w', 'sum_wf')))


# ------------------------------------------------------------------ the cases: name -> (la, lb, w, f), planes of one range
def scaled(rng, shape, dtype=np.float64, spread=20):
    """signed values with full mantissas and exponents in [-spread, spread)"""
    v = np.ldexp(rng.uniform(1.0, 2.0, shape), rng.integers(-spread, spread, shape)) * rng.choice([-1.0, 1.0], shape)
    return v.astype(dtype)


def blobs(rng, ny, nx, nlab, fill=0.5):
    """a map of rectangles of labels over -1"""
    m = np.full((ny, nx), -1, dtype=np.int32)
    for p in range(nlab):
        r, c = int(rng.integers(0, ny)), int(rng.integers(0, nx))
        h, w = int(rng.integers(1, max(2, int(ny * fill)))), int(rng.integers(1, max(2, int(nx * fill))))
        m[r:r + h, c:c + w] = p
    return m


def stripes():
    """65 x 65: one stripe per row against one stripe per column -- 4 225 distinct pairs, every node starts a run"""
    return (np.repeat(np.arange(65, dtype=np.int32)[:, None], 65, axis=1), np.repeat(np.arange(65, dtype=np.int32)[None, :], 65, axis=0))


def cases():
    rng = np.random.default_rng(2200)
    out = {}
    none = np.full((20, 70), -1, dtype=np.int32)
    out['both all -1'] = (none, none.copy(), None, None)
    m = blobs(rng, 40, 70, 9)
    out['identical maps'] = (m, m.copy(), scaled(rng, m.shape), scaled(rng, m.shape))
    sa, sb = stripes()
    out['stripes'] = (sa, sb, scaled(rng, sa.shape), None)
    a, b = np.full((70, 130), 3, dtype=np.int32), np.full((70, 130), 5, dtype=np.int32)
    b[37, 64] = 6
    out['one pair but one node'] = (a, b, scaled(rng, a.shape), scaled(rng, a.shape, np.float32))
    a = blobs(rng, 33, 65, 5)
    a[a == 0] = 2 ** 31 - 1
    a[a == 1] = 0
    out['labels 2^31 - 1 and 0'] = (a, blobs(rng, 33, 65, 4), None, scaled(rng, a.shape))
    a, b = blobs(rng, 33, 65, 6), blobs(rng, 33, 65, 6)
    a[a == 2] = -7
    b[b == 3] = np.iinfo(np.int32).min
    a[5:9, 5:9], b[5:9, 5:9] = -7, 4                                         # (-7, 4): a row (-1, 4)
    out['labels -7 and INT32_MIN'] = (a, b, scaled(rng, a.shape), None)
    a, b = blobs(rng, 40, 70, 8), blobs(rng, 40, 70, 8)
    a[:, 0], b[:, 0] = -1, 2                                                  # rows (-1, 2) whatever the blobs do
    a[0, 1:9], b[0, 1:9] = 2, 1                                               # (2, 1) and (1, 2): an ordered key
    a[1, 1:5], b[1, 1:5] = 1, 2
    out['blobs'] = (a, b, scaled(rng, a.shape), scaled(rng, a.shape))
    # a pair whose only run crosses no chunk boundary and ends with its chunk: lost without the flush
    a, b = np.full((40, 9), -1, dtype=np.int32), np.full((40, 9), -1, dtype=np.int32)
    a[3:5, 4], b[3:5, 4] = 1, 7
    out['one short run'] = (a, b, None, None)
    # weights over 2^+-40 with cancellation: inside the 160-bit window (its edges: test_gpu_ring_sums.py, on ring_sums_cases.py)
    a, b = blobs(rng, 33, 64, 4), blobs(rng, 33, 64, 3)
    w = scaled(rng, a.shape, spread=40)
    w[:, 1::2] = -w[:, 0::2]
    w[0, :] = scaled(rng, (64,), spread=40)
    out['cancellation'] = (a, b, w, scaled(rng, a.shape, spread=10))
    return out


BROKEN = ('no flush at the chunk\'s end', 'one-sided rows dropped', 'negative labels kept', 'unordered key')
