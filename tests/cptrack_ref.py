"""Restatements of K23 (xc_ring_tracks_dev) in plain Python, from the header's rule (include/xcontour_hip.h, K23 section) -- a helper for the
tests, no tests here.

accepted()       the accept rule: a >= 0, b >= 0, n >= 1 and float(n) >= min_overlap * float(min(size[a], size[b])), one product.
tracks_of()      the SET rule: a union-find over the accepted links whose root is the component's minimum; the dense ranks of the roots, the
                 degrees and the track rows from their definitions.
rounds_of()      what the kernels do instead: parent[g] <= g, rounds of hook (every accepted link reads both roots from the parents as the
                 round found them and takes the minimum of the smaller root into the larger root's parent) and compress, until a round
                 changes nothing -> (root, rounds).  `broken` names a deliberate defect (test_cptrack_host.py shows that the cases of the
                 GPU record test catch each of BROKEN, test_cptrack_geometry_host.py that those of cptrack_geometry_cases.py catch each
                 of BROKEN_GEOMETRY).
refused()        the index check: which link arrays the call refuses.
tracks_of_rows() the facade's view of one level of one series: K22's rows of every pair of consecutive steps -> per step the rings'
                 track / nprev / nnext, per step the rows' `linked`, and the track table.
cases()          the hand-built graphs of tests/test_gpu_cptrack_records.py.
scene()          the drifting Gaussian blobs of tests/test_gpu_cptrack.py."""
import numpy as np

ROW_DTYPE = np.dtype([('first_ring', np.int64), ('first_step', np.int32), ('last_step', np.int32), ('nrings', np.int64), ('nsplit', np.int64),
                      ('nmerge', np.int64)])
TRACK_DTYPE = np.dtype([('first_step', np.int32), ('first_row', np.int64), ('last_step', np.int32), ('nrings', np.int64), ('nsplit', np.int64),
                        ('nmerge', np.int64)])
BROKEN = ('no compression', 'smaller root under the larger', 'threshold > instead of >=', 'degrees counted on rejected links')
# ... and those that only the graphs of cptrack_geometry_cases.py tell apart (test_cptrack_geometry_host.py names the case for each); kept
# beside BROKEN, which test_cptrack_host.py walks with a table of its own.  The last one is a defect of refused(), not of tracks_of().
BROKEN_GEOMETRY = ('first_step from the root', 'last_step from the last ring', 'nsplit counts links', 'max size in the threshold',
                   'n >= 0 accepted', 'only a checked against nring')


def accepted(size, la, lb, ln, min_overlap, broken=None):
    la, lb, ln = (np.asarray(v, dtype=np.int64) for v in (la, lb, ln))
    ok = (la >= 0) & (lb >= 0) & (ln >= (0 if broken == 'n >= 0 accepted' else 1))
    if min_overlap != 0:
        size = np.asarray(size, dtype=np.int64)
        pick = max if broken == 'max size in the threshold' else min
        for i in np.flatnonzero(ok).tolist():
            need = float(min_overlap) * float(pick(int(size[la[i]]), int(size[lb[i]])))     # one float64 product
            ok[i] = float(int(ln[i])) > need if broken == 'threshold > instead of >=' else float(int(ln[i])) >= need
    return ok


def refused(nring, la, lb, broken=None):
    """the index check: any link with a >= nring or b >= nring refuses the call, whatever its other index and its n are"""
    la, lb = np.asarray(la, dtype=np.int64), np.asarray(lb, dtype=np.int64)
    return bool((la >= nring).any()) if broken == 'only a checked against nring' else bool(((la >= nring) | (lb >= nring)).any())


def degrees(nring, la, lb, ok, broken=None):
    la, lb = np.asarray(la, dtype=np.int64), np.asarray(lb, dtype=np.int64)
    if broken == 'degrees counted on rejected links':
        ok = (la >= 0) & (lb >= 0)
    nprev, nnext = np.zeros(nring, dtype=np.int32), np.zeros(nring, dtype=np.int32)
    np.add.at(nnext, la[ok], 1)
    np.add.at(nprev, lb[ok], 1)
    return nprev, nnext


def union_find(nring, la, lb, ok):
    """-> root (nring,): the smallest ring of every ring's component"""
    parent = list(range(nring))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r
    for a, b in zip(np.asarray(la)[ok].tolist(), np.asarray(lb)[ok].tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(g) for g in range(nring)], dtype=np.int64)


def rows_of(root, step, nprev, nnext, broken=None):
    """-> (track (nring,), the rows (ROW_DTYPE)) from the roots, by their definitions"""
    step, nnext = np.asarray(step), np.asarray(nnext)
    roots = np.unique(root)
    track = np.searchsorted(roots, root).astype(np.int64)
    rows = np.zeros(roots.size, dtype=ROW_DTYPE)
    rows['first_ring'] = roots
    rows['first_step'], rows['last_step'] = np.iinfo(np.int32).max, np.iinfo(np.int32).min
    first, last = rows['first_step'].copy(), rows['last_step'].copy()
    np.minimum.at(first, track, step)
    np.maximum.at(last, track, step)
    rows['first_step'], rows['last_step'] = first, last
    rows['nrings'] = np.bincount(track, minlength=roots.size)
    rows['nsplit'] = np.bincount(track[nnext >= 2], minlength=roots.size)
    rows['nmerge'] = np.bincount(track[np.asarray(nprev) >= 2], minlength=roots.size)
    if broken == 'first_step from the root':
        rows['first_step'] = step[roots]
    if broken == 'last_step from the last ring':
        largest = np.zeros(roots.size, dtype=np.int64)
        np.maximum.at(largest, track, np.arange(track.size))
        rows['last_step'] = step[largest]
    if broken == 'nsplit counts links':
        rows['nsplit'] = np.bincount(track[nnext >= 2], weights=nnext[nnext >= 2], minlength=roots.size).astype(np.int64)
    return track, rows


def tracks_of(nring, step, size, la, lb, ln, min_overlap=0.0, broken=None, root=None):
    """the rule -> dict(root, track, nprev, nnext, link_ok, rows); root: another one than the union-find's (rounds_of's)"""
    ok = accepted(size, la, lb, ln, min_overlap, broken)
    nprev, nnext = degrees(nring, la, lb, ok, broken)
    if root is None:
        root = union_find(nring, la, lb, ok)
    track, rows = rows_of(root, np.asarray(step), nprev, nnext, broken)
    return dict(root=root, track=track, nprev=nprev, nnext=nnext, link_ok=ok, rows=rows)


def rounds_of(nring, la, lb, ok, broken=None):
    """the kernels' rounds -> (root, rounds: the last, unchanged one included; 0 without links)"""
    la, lb = np.asarray(la, dtype=np.int64)[ok], np.asarray(lb, dtype=np.int64)[ok]
    parent = np.arange(nring, dtype=np.int64)
    up = broken == 'smaller root under the larger'

    def find(p, x):
        x = x.copy()
        while True:
            nxt = p[x]
            if (nxt == x).all():
                return x
            x = nxt
    rounds = 0
    changed = np.asarray(ok).size > 0
    while changed:
        assert rounds <= nring, 'more than nring + 1 rounds'
        ra, rb = find(parent, la), find(parent, lb)                          # both roots, as the round found the parents
        diff = ra != rb
        changed = bool(diff.any())
        lo, hi = np.minimum(ra, rb)[diff], np.maximum(ra, rb)[diff]
        if up:
            np.maximum.at(parent, lo, hi)
        else:
            np.minimum.at(parent, hi, lo)                                     # atomicMin(&parent[larger], smaller)
        if broken != 'no compression':
            parent = find(parent, np.arange(nring, dtype=np.int64))
        rounds += 1
    return parent, rounds


def same(got, ref):
    """every word equal: the five per-ring / per-link arrays and the rows"""
    return (all(np.array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(ref[k]).astype(np.int64))
                for k in ('root', 'track', 'nprev', 'nnext', 'link_ok'))
            and got['rows'].size == ref['rows'].size and all(np.array_equal(got['rows'][k], ref['rows'][k]) for k in ROW_DTYPE.names))


# ------------------------------------------------------------------ one level of one series, as the facade returns it
def tracks_of_rows(counts, sizes, rows, min_overlap=0.0):
    """counts[t]: the rings of step t; sizes[t]: their nodes_net; rows[t]: K22's rows (fields a, b, and n or nodes) of step t against
    t + 1 -> (per step track / nprev / nnext arrays, per step the rows' linked, the tracks (TRACK_DTYPE))"""
    counts = np.asarray(counts, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(counts)])
    nring = int(off[-1])
    step = np.repeat(np.arange(counts.size), counts).astype(np.int32)
    size = np.concatenate([np.asarray(s, dtype=np.int64) for s in sizes]) if nring else np.empty(0, dtype=np.int64)
    la, lb, ln = [], [], []
    for t, r in enumerate(rows):
        n = r['n'] if 'n' in r.dtype.names else r['nodes']
        la.append(np.where(r['a'] >= 0, off[t] + r['a'], -1))
        lb.append(np.where(r['b'] >= 0, off[t + 1] + r['b'], -1))
        ln.append(n)
    la, lb, ln = (np.concatenate(v).astype(np.int64) if v else np.empty(0, dtype=np.int64) for v in (la, lb, ln))
    t = tracks_of(nring, step, size, la, lb, ln, min_overlap)
    cut = lambda v, o: [v[o[k]:o[k + 1]] for k in range(len(o) - 1)]
    loff = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64)
    table = np.empty(t['rows'].size, dtype=TRACK_DTYPE)
    for k in ('first_step', 'last_step', 'nrings', 'nsplit', 'nmerge'):
        table[k] = t['rows'][k]
    table['first_row'] = t['rows']['first_ring'] - off[t['rows']['first_step']]
    return dict(track=cut(t['track'], off), nprev=cut(t['nprev'], off), nnext=cut(t['nnext'], off), linked=cut(t['link_ok'], loff),
                tracks=table)


# ------------------------------------------------------------------ the hand-built graphs: name -> dict(nring, step, size, la, lb, ln, mo)
def graph(nring, links, step=None, size=None, mo=0.0):
    links = np.asarray(links, dtype=np.int64).reshape(-1, 3)
    step = np.arange(nring, dtype=np.int32) if step is None else np.asarray(step, dtype=np.int32)
    return dict(nring=nring, step=step, size=None if size is None else np.asarray(size, dtype=np.int64), la=links[:, 0].copy(),
                lb=links[:, 1].copy(), ln=links[:, 2].copy(), mo=mo)


def chain(n, order):
    links = np.stack([np.arange(n - 1), np.arange(1, n), np.ones(n - 1, dtype=np.int64)], axis=1)
    if order == 'reversed':
        links = links[::-1]
    if order == 'shuffled':
        links = links[np.random.default_rng(2305).permutation(n - 1)]
    return graph(n, links)


def random_graph(rng, nring, nlink, nstep=40, thresholds=True):
    """rings on `nstep` steps, links from a step to the next; every tenth link has a -1 or n = 0; sizes and n spread round the threshold"""
    step = np.sort(rng.integers(0, nstep, nring)).astype(np.int32)
    la = rng.integers(0, nring, nlink)
    lb = np.minimum(la + rng.integers(1, max(2, nring // nstep), nlink), nring - 1)
    ln = rng.integers(1, 12, nlink)
    odd = rng.integers(0, 30, nlink)
    la[odd == 0], lb[odd == 1], ln[odd == 2] = -1, -1, 0
    size = rng.integers(1, 24, nring)
    return graph(nring, np.stack([la, lb, ln], axis=1), step=step, size=size, mo=0.5 if thresholds else 0.0)


def cases():
    rng = np.random.default_rng(2300)
    out = {'one ring, no link': graph(1, [])}
    for nring in (255, 256, 257):
        for nlink in (1, 255, 257):
            out['%d rings, %d links' % (nring, nlink)] = random_graph(rng, nring, nlink, nstep=8, thresholds=nlink != 255)
    for order in ('ascending', 'reversed', 'shuffled'):
        out['chain of 5000, %s' % order] = chain(5000, order)
    out['diamond'] = graph(5, [(0, 1, 3), (0, 2, 2), (1, 3, 3), (2, 3, 1)], step=[0, 1, 1, 2, 2])       # ring 4: a track of one
    # rings 0, 2, 4, ... and 1, 3, 5, ...: two chains whose LAST rings alone are linked: one track, rooted in ring 0
    n = 301
    links = [(g, g + 2, 1) for g in range(n - 2)] + [(n - 2, n - 1, 1)]
    out['two chains that meet at their last rings'] = graph(n, links[::-1], step=np.arange(n) // 2)
    out['duplicate links'] = graph(4, [(0, 1, 2), (0, 1, 2), (0, 1, 5), (2, 3, 1), (2, 3, 1)], step=[0, 1, 0, 1])
    out['-1 on either side'] = graph(5, [(-1, 1, 4), (0, -1, 4), (-1, -1, 4), (2, 3, 4), (-7, 4, 1)], step=[0, 1, 0, 1, 1])
    out['n == 0'] = graph(4, [(0, 1, 0), (2, 3, 1), (0, 3, -2)], step=[0, 1, 0, 1])
    # 0.5 * 8 = 4.0: met exactly by n = 4, missed by one node by n = 3; 0.07 * 100 rounds to 7.000000000000001: n = 7 misses it, n = 8 meets it
    out['the threshold met exactly and missed by one'] = graph(
        8, [(0, 1, 4), (2, 3, 3), (4, 5, 50), (6, 7, 49)], step=[0, 1] * 4, size=[8, 30, 30, 8, 100, 200, 200, 100], mo=0.5)
    out['the threshold is one rounded product'] = graph(4, [(0, 1, 7), (2, 3, 8)], step=[0, 1] * 2, size=[100, 200, 200, 100], mo=0.07)
    out['no sizes, min_overlap 0'] = graph(6, [(0, 1, 1), (1, 2, 1), (3, 4, 1), (0, 2, 1)], step=[0, 1, 2, 0, 1, 2])
    out['min_overlap 1'] = graph(4, [(0, 1, 5), (2, 3, 4)], step=[0, 1] * 2, size=[5, 9, 5, 9], mo=1.0)
    out['100 000 rings, 150 000 links'] = random_graph(rng, 100000, 150000, nstep=400)
    return out


# ------------------------------------------------------------------ the scene of the facade test
NY, NX, NSTEP = 24, 48, 12
LEVELS = np.array([0.3, 0.5, 0.7])


def scene(nstep=NSTEP):
    """drifting Gaussian blobs on a periodic 24 x 48 plane, float64 (nstep, 24, 48); rows 0 and 23 lie below every level.
    A drifts east across the seam; B stands and C comes up to it, merges with it and leaves it again; D is born at step 4; E exists at
    step 7 alone; F runs so fast that its consecutive rings share only a few nodes."""
    y, x = np.arange(NY)[:, None], np.arange(NX)[None, :]

    def blob(cy, cx, sig, amp=1.0):
        dx = (x - cx + NX / 2.0) % NX - NX / 2.0
        return amp * np.exp(-((y - cy) ** 2 + dx ** 2) / (2.0 * sig * sig))
    q = np.zeros((nstep, NY, NX))
    for t in range(nstep):
        q[t] += blob(5.0, 43.0 + 0.9 * t, 2.2)                                # A
        q[t] += blob(12.0, 12.0, 2.4)                                         # B
        q[t] += blob(12.5, 24.0 - 1.6 * min(t, 11 - t), 2.2)                  # C: 24 -> 16 -> 24
        if t >= 4:
            q[t] += blob(5.5, 20.0 + 0.3 * t, 2.0, min(1.0, 0.45 * (t - 3)))  # D
        if t == 7:
            q[t] += blob(5.0, 31.5, 1.8)                                      # E
        q[t] += blob(19.0, 6.0 + 3.4 * t, 1.9)                                # F
    q[:, 0], q[:, -1] = 0.0, 0.0
    return q
