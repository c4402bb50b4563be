"""K1 (xc_misc.hip k_minmax_partial) restated on the host: how one launch cuts every slab into a scalar head, a body of 16-byte vectors
dealt to P blocks, and scalar tails -- and from that the POSITIONS at which a planted extremum tells a kernel that reads all of a
slab from one that drops a part of it.  No GPU here; test_minmax_ref_host.py pins this module, test_gpu_minmax_geometry.py uses it.

The kernel, per slab s of a launch of `nslab` slabs of `ncell` cells whose pointer lies `mis` elements behind a 16-byte boundary:
  start = (mis + s * ncell) mod VN              VN = 4 float32 / 2 float64 cells in 16 bytes
  head  = min((VN - start) mod VN, ncell)       scalar cells [0, head), read by block 0
  nvec  = (ncell - head) div VN                 vectors; vector v holds the cells head + v * VN + (0 .. VN - 1)
  per   = ceil(nvec / P)                        P = minmax_blocks(ncell, nslab); block b owns the vectors [b * per, min(b * per + per, nvec))
  tail  = [head + nvec * VN, ncell)             scalar cells, read by block 0
Inside a block of L vectors thread t starts at vector t and takes BATCHES of 8 loads (t + 256 u, u = 0 .. 7) while t + 2048 k + 1792 < L,
then single loads every 256 vectors (the remainder loop)."""
import numpy as np

THREADS, UNROLL = 256, 8
BATCH = THREADS * UNROLL
SLOTS = (0, 3, 7)                                # the load slots of a batch that get a class of their own


def minmax_blocks(ncell, nslab=1):
    """xc_internal.h minmax_blocks(): K1 blocks per slab.  About 8192 cells a block, at most 1024; a launch of fewer than 2048 blocks
    in all takes 4096 cells a block instead, as far as 2048 blocks in all go"""
    p = (ncell + 8191) // 8192
    if p > 1024:
        p = 1024
    if nslab < 1:
        nslab = 1
    if p * nslab < 2048:
        f = (ncell + 4095) // 4096
        if f * nslab > 2048:
            f = 2048 // nslab
        if f > p:
            p = f
    return 1 if p < 1 else (2048 if p > 2048 else p)


class Partition(object):
    """slab `s` of one launch (see the module's text).  blocks: [(v0, v1)] of all P blocks, v1 <= v0 for a block without vectors"""

    def __init__(self, itemsize, ncell, nslab, mis, s):
        self.vn = vn = 16 // itemsize
        assert itemsize in (4, 8) and 0 <= mis < vn and 0 <= s < nslab and ncell >= 1
        self.ncell, self.P = ncell, minmax_blocks(ncell, nslab)
        start = (mis + s * ncell) % vn
        self.head = min((vn - start) % vn, ncell)
        self.nvec = (ncell - self.head) // vn
        self.per = -(-self.nvec // self.P)
        self.blocks = [(b * self.per, min(b * self.per + self.per, self.nvec)) for b in range(self.P)]
        self.tail = (self.head + self.nvec * vn, ncell)

    def cell(self, v, c):
        return self.head + v * self.vn + c

    def nonempty(self):
        return [b for b, (v0, v1) in enumerate(self.blocks) if v1 > v0]


def in_batch(L, j):
    """is vector j (counted from the block's first) of a block of L vectors loaded by the unrolled loop?  (array or int j)"""
    return j % THREADS + BATCH * (j // BATCH) + (UNROLL - 1) * THREADS < L


def batch_threads(L):
    """threads [0, n) take at least one unrolled batch in a block of L vectors"""
    return max(0, min(THREADS, L - (UNROLL - 1) * THREADS))


def remainder_threads(L):
    """sorted thread indices that take at least one step of the remainder loop in a block of L vectors"""
    j = np.arange(L)
    return np.unique(j[~in_batch(L, j)] % THREADS).tolist()


def classes(p):
    """{name: cell index in the slab} of partition p: every position class that exists in it (two names may share a cell)"""
    out = {}
    for j in range(p.head):
        out['head[%d]' % j] = j
    for j in range(p.tail[0], p.tail[1]):
        out['tail[%d]' % (j - p.tail[0])] = j
    ne = p.nonempty()
    picks = [('first', ne[0])] if ne else []
    if len(ne) >= 3:
        picks.append(('middle', ne[len(ne) // 2]))
    if len(ne) >= 2:
        picks.append(('last', ne[-1]))
    for tag, b in picks:
        v0, v1 = p.blocks[b]
        L = v1 - v0
        for end, v in (('first', v0), ('last', v1 - 1)):
            for c in range(p.vn):
                out['%s block, %s vector, c%d' % (tag, end, c)] = p.cell(v, c)
        nb = batch_threads(L)
        if nb:
            for tname, t in (('first', 0), ('last', nb - 1)):
                nbatch = -(-(L - (UNROLL - 1) * THREADS - t) // BATCH)           # batches of thread t
                for bname, k in (('first', 0), ('last', nbatch - 1)):
                    if bname == 'last' and nbatch == 1:
                        continue
                    for u in SLOTS:
                        j = t + BATCH * k + THREADS * u
                        assert j < L and in_batch(L, j)
                        out['%s block, %s batch, %s thread, u%d' % (tag, bname, tname, u)] = p.cell(v0 + j, (u + t) % p.vn)
        j = np.arange(L)
        rem = j[~in_batch(L, j)]
        if rem.size:
            out['%s block, remainder, first vector' % tag] = p.cell(v0 + int(rem[0]), 0)
            out['%s block, remainder, last vector' % tag] = p.cell(v0 + int(rem[-1]), p.vn - 1)
    for b in ne[1:]:
        v0 = p.blocks[b][0]
        out['cut %d, before' % b] = p.cell(v0 - 1, p.vn - 1)
        out['cut %d, after' % b] = p.cell(v0, 0)
    assert all(0 <= c < p.ncell for c in out.values())
    return out


def launch_classes(itemsize, ncell, nslab, mis):
    """[classes of slab s] of one launch"""
    return [classes(Partition(itemsize, ncell, nslab, mis, s)) for s in range(nslab)]


def schedule(per_slab):
    """Deal the classes of a launch to calls: [[(max name or None, min name or None) per slab] per call], so that over the calls every
    name that exists in any slab carries the maximum of some slab once and the minimum of some slab once, never both on one cell.
    Slab s starts looking at its class s mod nclass (the maximum) and walks the minimum the other way: one call of many slabs covers
    all classes, a launch of two slabs takes as many calls as it needs."""
    names = sorted(set(n for c in per_slab for n in c))
    need = [set(names), set(names)]
    calls = []
    while need[0] or need[1]:
        call, before = [], len(need[0]) + len(need[1])
        for s, c in enumerate(per_slab):
            own = [n for n in names if n in c]
            k = s % max(len(own), 1)
            fwd, back = own[k:] + own[:k], (own[k:] + own[:k])[::-1]
            a = next((n for n in fwd if n in need[0]), None)
            b = next((n for n in back if n in need[1] and (a is None or c[n] != c[a])), None)
            need[0].discard(a)
            need[1].discard(b)
            call.append((a, b))
        # (a call always gets on: a name that still wants the maximum is taken by a slab that has it, and once none does every slab
        # is free to take any minimum)
        assert len(need[0]) + len(need[1]) < before
        calls.append(call)
    return calls


# ------------------------------------------------------------------ the shapes of test_gpu_minmax_geometry.py, smallest per regime
SMALL = [(5, 1), (5, 2), (5, 7), (5, 77)]                                    # (nslab, ncell): head, tail, empty or tiny body
ONE_BLOCK = (2, 1023)
SHORT_LAST = (3, 16381)
F64_BOTH = (700, 9001)
F32_UNROLLED = (700, 15001)
MANY_BLOCKS = (2, 1228803)
SHAPES = SMALL + [ONE_BLOCK, SHORT_LAST, F64_BOTH, F32_UNROLLED, MANY_BLOCKS]
FINAL_BLOCKS = (0, 255, 256, 300)                                            # where k_minmax_final's second step is pinned (P = 301)


def misalignments(itemsize):
    return range(16 // itemsize)
