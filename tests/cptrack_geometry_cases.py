"""The ring graphs behind test_gpu_cptrack_geometry.py, shared with test_cptrack_geometry_host.py -- a helper, no tests here.
cptrack_ref.cases() shows that K23's RULE is right on graphs whose steps ascend with the ring index and whose links run from a smaller
ring to a larger one; these graphs sit where its MAPPING (xc_cptrack.hip) can go wrong unseen: the row reductions (atomicMin / atomicMax
with hand-set initial words) on steps in any order and over all of int32, links with a > b and a == b (parent[g] <= g rests on the hook
taking the SMALLER root, not a's), a chain that needs many rounds of the host loop, rings of degree 70 000 (one word takes every degree
atomic and every hook of a round), the dense rank of the roots on both sides of a wave of 64 and a block of 256 rings, calls without
links and with every link rejected, the conversions of the accept rule, and the second trip of the five grid-stride loops.

cases(): name -> a cptrack_ref.graph (nring, step, size, la, lb, ln, mo) with
  tag      what the case sits on, in words
  want     the answers written out, where the case has them: any of root, track, nprev, nnext, link_ok (lists), rows (tuples of
           cptrack_ref.ROW_DTYPE) and first_ring
  group    'steps', 'direction', 'hub', 'rank', 'rejected', 'accept'
second_trip() / second_trip_chained(): the graphs of more than RT_MAX_BLOCKS * RT_TPB rings and links with their closed-form answers.
refusals(): name -> (case, link, (a, b, n)): one link of a case replaced by one the index check must refuse.
The expected values of the GPU tests come from cptrack_ref.tracks_of, for the two large graphs from the closed forms here (which
test_cptrack_geometry_host.py checks against tracks_of at a small size)."""
import functools

import numpy as np

import cptrack_ref as KR

RT_TPB, RT_MAX_BLOCKS = 256, 1 << 16          # xc_cptrack.hip: the threads of a block and the blocks of a grid-stride launch
STRIDE = RT_TPB * RT_MAX_BLOCKS                # 2^24: the first ring / link of a second trip
TAIL = 300                                     # ... and how many of them the large graphs have
I32 = np.iinfo(np.int32)
STEP_BASES = ('257 rings, 257 links', '100 000 rings, 150 000 links')
ISOLATED = (2, 63, 64, 65, 255, 256, 257, 1000)
# the roots of the 1024-ring graphs.  Ring 0 is the smallest ring of its component in any graph, so it is a root beside the chosen ones.
ROOT_SETS = {'{0}': [0], '{63, 64}': [63, 64], '{255, 256}': [255, 256], '{0, 511, 512, 1023}': [0, 511, 512, 1023],
             'every ring': list(range(1024)), 'block 3 alone': list(range(768, 1024))}
HUB_N = 70000


def tagged(g, group, tag, **want):
    return dict(g, group=group, tag=tag, want=want)


def reference(c, broken=None, root=None):
    return KR.tracks_of(c['nring'], c['step'], c['size'], c['la'], c['lb'], c['ln'], c['mo'], broken=broken, root=root)


def rounds_fixed(c, ref):
    """the rounds the header fixes: 0 without links; 1 when no accepted link joins two different rings (every link rejected, or accepted
    self links alone: the first round changes nothing); None otherwise: at least 2 -- a last round changes nothing -- and at most nring + 1"""
    if c['la'].size == 0:
        return 0
    return None if (ref['link_ok'] & (c['la'] != c['lb'])).any() else 1


def shuffled(c, seed=2312):
    """the same graph with its links in another order"""
    p = np.random.default_rng(seed).permutation(c['la'].size)
    return dict(c, la=c['la'][p], lb=c['lb'][p], ln=c['ln'][p]), p


def with_link(c, at, link):
    out = dict(c, la=c['la'].copy(), lb=c['lb'].copy(), ln=c['ln'].copy())
    out['la'][at], out['lb'][at], out['ln'][at] = link
    return out


# ------------------------------------------------------------------ 1. steps in any order
def wide_steps(base, seed):
    """steps drawn from all of int32; INT32_MIN on the largest ring of a track of two or more rings, INT32_MAX on the root of another"""
    rng = np.random.default_rng(seed)
    step = rng.integers(I32.min, I32.max, base['nring'], endpoint=True).astype(np.int32)
    t = reference(base)
    many = np.flatnonzero(t['rows']['nrings'] >= 2)
    assert many.size >= 2
    for track, at, v in ((many[0], -1, I32.min), (many[-1], 0, I32.max)):
        step[np.flatnonzero(t['track'] == track)[at]] = v
    return step


def step_cases(out):
    base = KR.cases()
    for k, name in enumerate(STEP_BASES):
        b = base[name]
        perm = np.random.default_rng(2313 + k).permutation(b['step'])
        out['%s, steps permuted' % name] = tagged(dict(b, step=perm), 'steps', 'the same steps on other rings: no order between ring and step')
        out['%s, steps over all of int32' % name] = tagged(dict(b, step=wide_steps(b, 2315 + k)), 'steps',
                                                             'negative steps, INT32_MIN and INT32_MAX, the initial words of the rows')
    # rings 0 .. 3 one track: its root has step 5, its largest ring step 7, its min -3 and its max 9 lie between; ring 4 alone
    out['five rings, steps out of order'] = tagged(
        KR.graph(5, [(0, 1, 1), (1, 2, 1), (2, 3, 1)], step=[5, -3, 9, 7, 2]), 'steps', 'first_step and last_step of neither end of the track',
        root=[0, 0, 0, 0, 4], track=[0, 0, 0, 0, 1], rows=[(0, -3, 9, 4, 0, 0), (4, 2, 2, 1, 0, 0)])


# ------------------------------------------------------------------ 2. links in either direction
def direction_cases(out):
    n = 5000
    p = np.random.default_rng(2311).permutation(n)
    one = np.ones(n - 1, dtype=np.int64)
    out['chain of 5000, labels permuted'] = tagged(KR.graph(n, np.stack([p[:-1], p[1:], one], axis=1)), 'direction',
                                                   'half of the links have a > b; 9 synchronous rounds')
    g = np.arange(n - 1)
    out['chain of 5000, descending'] = tagged(KR.graph(n, np.stack([g + 1, g, one], axis=1)), 'direction', 'every link has a > b')
    # ring g has the link (g, g); every seventh ring twice
    g = np.arange(600)
    own = np.concatenate([g, g[::7]])
    twice = [2 if k % 7 == 0 else 1 for k in range(600)]
    out['600 rings, self links only'] = tagged(
        KR.graph(600, np.stack([own, own, np.ones(own.size, dtype=np.int64)], axis=1)), 'direction', 'a == b: a degree on both sides, no hook',
        root=list(range(600)), track=list(range(600)), nprev=twice, nnext=twice,
        rows=[(k, k, k, 1, int(k % 7 == 0), int(k % 7 == 0)) for k in range(600)])
    d = KR.cases()['diamond']
    links = np.stack([d['la'], d['lb'], d['ln']], axis=1).tolist()
    links = links[:2] + [(0, 0, 1), (3, 3, 2)] + links[2:] + [(4, 4, 1), (4, 4, 1)]
    out['diamond with self links'] = tagged(
        KR.graph(5, links, step=d['step']), 'direction', 'self links between the links of a merger and a split',
        root=[0, 0, 0, 0, 4], track=[0, 0, 0, 0, 1], nprev=[1, 1, 1, 3, 2], nnext=[3, 1, 1, 1, 2], link_ok=[True] * 8,
        rows=[(0, 0, 2, 4, 1, 1), (4, 2, 2, 1, 1, 1)])


# ------------------------------------------------------------------ 3. hubs
def hub(n, at, side):
    """ring `at` linked with every other ring, as a (side 'a') or as b; every third link twice, next to its first copy"""
    others = np.delete(np.arange(n), at)
    others = np.repeat(others, np.where(np.arange(n - 1) % 3 == 0, 2, 1))
    here = np.full(others.size, at)
    a, b = (here, others) if side == 'a' else (others, here)
    return KR.graph(n, np.stack([a, b, np.ones(others.size, dtype=np.int64)], axis=1), step=np.arange(n) % 1000)


def hub_cases(out):
    for at in (0, HUB_N - 1):
        for side in 'ab':
            out['hub %d of 70 000 as %s' % (at, side)] = tagged(
                hub(HUB_N, at, side), 'hub', 'every degree atomic on one word, every hook of a round on one parent; n%s counts rings'
                % ('split' if side == 'a' else 'merge'))


# ------------------------------------------------------------------ 4. the dense rank
def rooted(n, chosen):
    """n rings whose roots are `chosen` and ring 0: every other ring is linked with the ring before it"""
    roots = np.union1d(chosen, [0])
    g = np.setdiff1d(np.arange(n), roots)
    return KR.graph(n, np.stack([g - 1, g, np.ones(g.size, dtype=np.int64)], axis=1)), roots


def rank_cases(out):
    for n in ISOLATED:
        out['%d isolated rings' % n] = tagged(KR.graph(n, []), 'rank', 'no link: NULL link arrays, 0 rounds, every ring a root',
                                              root=list(range(n)), track=list(range(n)), first_ring=list(range(n)))
    for name, chosen in ROOT_SETS.items():
        g, roots = rooted(1024, chosen)
        track = np.searchsorted(roots, np.arange(1024), side='right') - 1
        out['1024 rings, roots %s' % name] = tagged(g, 'rank', 'roots on both sides of a wave / a block; blocks without a root',
                                                    root=roots[track].tolist(), track=track.tolist(), first_ring=roots.tolist())


# ------------------------------------------------------------------ 5. every link rejected
def rejected_case(out):
    n, nlink = 300, 400
    rng = np.random.default_rng(2317)
    a, b = rng.integers(0, n, nlink), rng.integers(0, n, nlink)
    ln = np.full(nlink, 9, dtype=np.int64)
    k = np.arange(nlink) % 4
    a[k == 0], b[k == 1], ln[k == 2], ln[k == 3] = -1, -1, 0, 4                # 4 < 0.5 * 10
    out['300 rings, 400 links, all rejected'] = tagged(
        KR.graph(n, np.stack([a, b, ln], axis=1), size=np.full(n, 10), mo=0.5), 'rejected', 'a = -1, b = -1, n == 0, under the threshold: 1 round',
        root=list(range(n)), track=list(range(n)), nprev=[0] * n, nnext=[0] * n, link_ok=[False] * nlink, first_ring=list(range(n)))


# ------------------------------------------------------------------ 6. the conversions of the accept rule
def accept_cases(out):
    two = 2 ** 53
    out['a size of 0'] = tagged(
        KR.graph(6, [(0, 1, 1), (2, 3, 1), (2, 3, 0), (4, 5, 2), (4, 5, 3)], step=[0, 1] * 3, size=[0, 7, 0, 0, 3, 3], mo=1.0), 'accept',
        'a threshold of 0 is met by any n >= 1 and by no n == 0', link_ok=[True, True, False, False, True], root=[0, 0, 2, 2, 4, 4])
    out['n greater than both sizes'] = tagged(
        KR.graph(4, [(0, 1, 9), (2, 3, 1 << 40)], step=[0, 1] * 2, size=[3, 5, 1 << 33, 1 << 32], mo=1.0), 'accept',
        'n is not clipped to a size', link_ok=[True, True], root=[0, 0, 2, 2])
    assert float(two + 1) == float(two) and float(two - 1) < float(two)
    out['n and size round 2^53'] = tagged(
        KR.graph(6, [(0, 1, two + 1), (2, 3, two - 1), (4, 5, two)], step=[0, 1] * 3, size=[two] * 4 + [two + 1] * 2, mo=1.0), 'accept',
        '(double)n and (double)size round to even: 2^53 + 1 meets 2^53, 2^53 - 1 misses it, 2^53 meets 2^53 + 1',
        link_ok=[True, False, True], root=[0, 0, 2, 3, 4, 4])


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    for add in (step_cases, direction_cases, hub_cases, rank_cases, rejected_case, accept_cases):
        add(out)
    return out


def refusals():
    """name -> (case, link, (a, b, n)): each is XC_EBADARG with nothing written"""
    hub_a = 'hub 0 of 70 000 as a'
    last = cases()[hub_a]['la'].size - 1
    return {'a bad b in the last link of a launch of many blocks': (hub_a, last, (0, HUB_N, 1)),
            'a negative a does not shield b == nring': ('diamond with self links', 1, (-1, 5, 3)),
            'a == nring on a link with n == 0': ('diamond with self links', 4, (5, 0, 0)),
            'b = 2^40': ('diamond with self links', 0, (0, 1 << 40, 3))}


# ------------------------------------------------------------------ 7. the second trip of the grid-stride loops
def pair_links(nring):
    half = nring // 2
    m = np.arange(nring, dtype=np.int64) % half
    return 2 * m, 2 * m + 1


def pair_steps(nring):
    g = np.arange(nring, dtype=np.int64)
    return ((g * 2654435761) % (1 << 32)).astype(np.uint32).view(np.int32)     # no order, both signs


def pair_rows(step, nprev, nnext, npair):
    """the rows of the pairs (2 t, 2 t + 1), t < npair"""
    rows = np.empty(npair, dtype=KR.ROW_DTYPE)
    s = step[:2 * npair].reshape(npair, 2)
    rows['first_ring'] = 2 * np.arange(npair, dtype=np.int64)
    rows['first_step'], rows['last_step'], rows['nrings'] = s.min(axis=1), s.max(axis=1), 2
    rows['nsplit'] = (nnext[:2 * npair].reshape(npair, 2) >= 2).sum(axis=1)
    rows['nmerge'] = (nprev[:2 * npair].reshape(npair, 2) >= 2).sum(axis=1)
    return rows


def second_trip(nring=STRIDE + TAIL):
    """nring rings in pairs (2 m, 2 m + 1), nring links: every pair linked twice, no sizes, min_overlap 0 -> (graph, answer).  With the
    default nring every grid-stride loop over rings or links takes a second trip of 300.  The answer is closed form: root = g & ~1,
    track = g >> 1, the degrees by bincount, the rows by reshape."""
    assert nring % 2 == 0
    la, lb = pair_links(nring)
    g = dict(nring=nring, step=pair_steps(nring), size=None, la=la, lb=lb, ln=np.ones(nring, dtype=np.int64), mo=0.0)
    ring = np.arange(nring, dtype=np.int64)
    nprev = np.bincount(lb, minlength=nring).astype(np.int32)
    nnext = np.bincount(la, minlength=nring).astype(np.int32)
    return g, dict(root=ring & ~1, track=ring >> 1, nprev=nprev, nnext=nnext, link_ok=np.ones(nring, dtype=bool),
                   rows=pair_rows(g['step'], nprev, nnext, nring // 2))


def second_trip_chained(nring=STRIDE + TAIL, first=STRIDE):
    """second_trip() with the links from `first` on replaced by a chain through the rings first .. nring - 1 and a link from its first ring
    to its last -> (graph, answer).  Those rings are ONE track that only links of the second trip join, that takes a compress of the
    second trip to flatten, and whose degrees only the accept of the second trip counts: second_trip() itself cannot tell a single-pass
    k_rt_accept, k_rt_hook or k_rt_compress, because its second-trip links repeat links of the first and join two roots directly."""
    assert nring % 2 == 0 and first % 2 == 0 and 2 < nring - first <= nring // 2
    g, _ = second_trip(nring)
    k = np.arange(nring - first - 1, dtype=np.int64)
    g['la'][first:], g['lb'][first:] = np.append(first + k, first), np.append(first + k + 1, nring - 1)
    ring = np.arange(nring, dtype=np.int64)
    nprev = np.bincount(g['lb'], minlength=nring).astype(np.int32)
    nnext = np.bincount(g['la'], minlength=nring).astype(np.int32)
    rows = np.empty(first // 2 + 1, dtype=KR.ROW_DTYPE)
    rows[:-1] = pair_rows(g['step'], nprev, nnext, first // 2)
    rows[-1] = (first, g['step'][first:].min(), g['step'][first:].max(), nring - first, (nnext[first:] >= 2).sum(), (nprev[first:] >= 2).sum())
    return g, dict(root=np.where(ring < first, ring & ~1, first), track=np.minimum(ring >> 1, first // 2), nprev=nprev, nnext=nnext,
                   link_ok=np.ones(nring, dtype=bool), rows=rows)


def tail_poison(nring=STRIDE + TAIL, first=STRIDE):
    """a graph of the same sizes whose call leaves ring 0 as the parent of the rings first .. nring - 1 in the workspace: what a k_rt_init
    that skips the second trip would then start from"""
    g, _ = second_trip(nring)
    g['la'][:], g['lb'][:], g['ln'][:] = -1, -1, 0
    n = nring - first
    g['la'][:n], g['lb'][:n], g['ln'][:n] = 0, first + np.arange(n), 1
    return g
