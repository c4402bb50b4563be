"""minmax_ref.py, the host restatement of K1's launch geometry, pinned without a GPU: minmax_blocks against values worked out by hand
from the C function's rule, the partition against a cell-by-cell replay of the kernel's loops, and -- for every shape that
test_gpu_minmax_geometry.py uses -- the regime the shape is there for and the position classes it yields, so that a later change of
minmax_blocks cannot silently empty a class."""
import numpy as np
import pytest

import minmax_ref as M
import sort_ref

# (ncell, nslab) -> P, by hand: p = min(ceil(ncell / 8192), 1024); if p * nslab < 2048: f = ceil(ncell / 4096), cut to 2048 div nslab
# when f * nslab > 2048, p = max(p, f)
BLOCKS = {(1, 1): 1, (4096, 1): 1, (4097, 1): 2, (8192, 1): 2, (77, 5): 1, (1023, 2): 1,
          (16381, 3): 4,               # p 2, f 4, 12 blocks in all
          (9001, 700): 2,              # p 2, f 3 -> 2048 div 700 = 2
          (15001, 700): 2,             # p 2, f 4 -> 2
          (1228803, 2): 301,           # p 151, f 301, 602 blocks in all
          (5000, 1000): 2,             # p 1, f 2, 2000 blocks in all
          (5000, 1025): 1,             # f 2 would make 2050 blocks: 2048 div 1025 = 1
          (5000, 3000): 1,             # p * nslab >= 2048: the coarse rule alone
          (100000, 65535): 13,
          (10 ** 7, 1): 2048,          # p 1221 -> 1024; f 2442 -> 2048
          (10 ** 7, 2): 1024,          # p * nslab = 2048 is not below 2048
          (2 ** 35, 1): 2048}


def test_minmax_blocks_equals_the_hand_table():
    for (ncell, nslab), P in BLOCKS.items():
        assert M.minmax_blocks(ncell, nslab) == P, (ncell, nslab)
        assert sort_ref.minmax_blocks(ncell, nslab) == P, (ncell, nslab)
    assert M.minmax_blocks(100, 0) == M.minmax_blocks(100, 1) == 1


def replay(itemsize, ncell, nslab, mis, s):
    """the kernel's loops, cell by cell: how often every cell of slab s is read, and which vectors (slab-wide index) the unrolled
    loop took with which (thread, slot)"""
    vn = 16 // itemsize
    P = M.minmax_blocks(ncell, nslab)
    addr = (mis + s * ncell) * itemsize
    head = min(((16 - (addr & 15)) & 15) // itemsize, ncell)
    nvec = (ncell - head) // vn
    per = (nvec + P - 1) // P
    reads, unrolled = np.zeros(ncell, dtype=np.int64), {}
    for b in range(P):
        v0 = b * per
        v1 = v0 + per if v0 + per < nvec else nvec
        for tid in range(256):
            i = v0 + tid
            while i + 7 * 256 < v1:
                for u in range(8):
                    v = i + u * 256
                    reads[head + v * vn:head + (v + 1) * vn] += 1
                    unrolled[v] = (tid, u)
                i += 8 * 256
            while i < v1:
                reads[head + i * vn:head + (i + 1) * vn] += 1
                i += 256
        if b == 0:
            reads[:head] += 1
            reads[head + nvec * vn:] += 1
    return reads, unrolled, head, nvec, per


@pytest.mark.parametrize('nslab,ncell', M.SMALL + [M.ONE_BLOCK, M.SHORT_LAST, (3, 9001), (3, 15001), (2, 40000)])
def test_partition_equals_a_replay_of_the_kernels_loops(nslab, ncell):
    for itemsize in (4, 8):
        for mis in M.misalignments(itemsize):
            for s in range(nslab):
                p = M.Partition(itemsize, ncell, nslab, mis, s)
                reads, unrolled, head, nvec, per = replay(itemsize, ncell, nslab, mis, s)
                assert (reads == 1).all(), 'the kernel itself reads every cell once'
                assert (p.head, p.nvec, p.per) == (head, nvec, per)
                assert p.tail == (head + nvec * p.vn, ncell) and p.tail[1] - p.tail[0] < p.vn
                got = {}
                for v0, v1 in p.blocks:
                    for j in range(max(0, v1 - v0)):
                        if M.in_batch(v1 - v0, j):
                            got[v0 + j] = (j % 256, (j % 2048) // 256)
                assert got == unrolled
                for v0, v1 in p.blocks:
                    L = max(0, v1 - v0)
                    took = sorted(set(t for v, (t, u) in unrolled.items() if v0 <= v < v1))
                    assert took == list(range(M.batch_threads(L)))
                    rem = sorted(set((v - v0) % 256 for v in range(v0, v1) if v not in unrolled))
                    assert rem == M.remainder_threads(L)
                for name, c in M.classes(p).items():
                    kind = 'head' if c < head else 'tail' if c >= p.tail[0] else 'batch' if (c - head) // p.vn in unrolled else 'remainder'
                    if name.startswith(('head', 'tail')) or ' batch, ' in name or ' remainder, ' in name:
                        assert kind in name, (name, kind)


def summary(itemsize, nslab, ncell):
    """what the launches of one shape reach, over every misalignment and slab"""
    parts = [M.Partition(itemsize, ncell, nslab, mis, s) for mis in M.misalignments(itemsize) for s in range(nslab)]
    names = set(n for p in parts for n in M.classes(p))
    return parts, names


def test_small_shapes_reach_every_head_and_tail_and_the_empty_body():
    for itemsize, vn in ((4, 4), (8, 2)):
        for nslab, ncell in M.SMALL:
            assert nslab >= 5
            parts, names = summary(itemsize, nslab, ncell)
            assert all(p.P == 1 for p in parts)
            assert set(p.head for p in parts) == set(range(min(vn, ncell + 1))), 'every head length'
            if ncell <= 2:
                assert any(p.nvec == 0 for p in parts), 'an empty body'
            if ncell == 7:
                assert all(1 <= p.nvec <= 3 for p in parts), 'a body of a vector or three'
        parts, names = summary(itemsize, 5, 77)
        assert set(p.tail[1] - p.tail[0] for p in parts) == set(range(vn)), 'every tail length'
        assert set('head[%d]' % j for j in range(vn - 1)) <= names and set('tail[%d]' % j for j in range(vn - 1)) <= names
        assert 'first block, remainder, last vector' in names and not any('batch' in n or 'cut' in n for n in names)
    # float32, two cells: head 2 / tail 0 and head 1 / tail 1 (and the whole slab a head of 2 cells behind 1 or 2 misaligned elements)
    got = set((p.head, p.tail[1] - p.tail[0], p.nvec) for p in summary(4, 5, 2)[0])
    assert {(2, 0, 0), (1, 1, 0), (0, 2, 0)} <= got


def test_one_block_takes_the_remainder_loop_only():
    for itemsize in (4, 8):
        parts, names = summary(itemsize, *M.ONE_BLOCK)
        assert all(p.P == 1 and len(p.nonempty()) == 1 for p in parts)
        assert all(M.batch_threads(p.nvec) == 0 for p in parts)
        assert all(len(M.remainder_threads(p.nvec)) == (256 if itemsize == 8 else 255) for p in parts), 'several steps of some threads'
        assert 'first block, last vector, c%d' % (16 // itemsize - 1) in names and not any('batch' in n or 'cut' in n for n in names)


def test_several_blocks_and_a_short_last_one():
    nslab, ncell = M.SHORT_LAST
    for itemsize in (4, 8):
        parts, names = summary(itemsize, nslab, ncell)
        for p in parts:
            assert p.P == 4 and len(p.nonempty()) == 4
            L = [v1 - v0 for v0, v1 in p.blocks]
            assert L[0] == L[1] == L[2] == p.per and 0 < L[3] < p.per, 'a short last block'
        for b in (1, 2, 3):
            assert {'cut %d, before' % b, 'cut %d, after' % b} <= names
        assert {'first block, first vector, c0', 'middle block, last vector, c1', 'last block, last vector, c0'} <= names
    for p in summary(8, nslab, ncell)[0]:                                      # float64: exactly one batch a thread, no remainder
        assert p.per == 2048 and M.batch_threads(2048) == 256 and M.remainder_threads(2048) == []
        assert len(M.remainder_threads(p.blocks[3][1] - p.blocks[3][0])) in (1, 2), 'the short block leaves a thread or two a single load'
    names = summary(8, nslab, ncell)[1]
    assert {'first block, first batch, first thread, u0', 'first block, first batch, last thread, u7',
            'last block, first batch, last thread, u3', 'last block, remainder, first vector'} <= names
    assert 'first block, remainder, first vector' not in names
    assert not any('batch' in n for n in summary(4, nslab, ncell)[1]), 'float32 stays in the remainder loop here'


def test_float64_unrolled_and_remainder_in_one_block():
    nslab, ncell = M.F64_BOTH
    parts, names = summary(8, nslab, ncell)
    for p in parts:
        assert (p.P, p.per) == (2, 2250) and p.nvec in (4500, 4499)
        assert M.batch_threads(2250) == 256 and M.remainder_threads(2250) == list(range(202))
    for tag in ('first', 'last'):
        assert {'%s block, first batch, last thread, u7' % tag, '%s block, remainder, first vector' % tag,
                '%s block, remainder, last vector' % tag} <= names
    assert {'head[0]', 'tail[0]', 'cut 1, before', 'cut 1, after'} <= names


def test_float32_reaches_the_unrolled_loop():
    nslab, ncell = M.F32_UNROLLED
    assert nslab * ncell * 4 < 128 << 20, 'below the size at which the launcher turns to the streaming loads by itself'
    parts, names = summary(4, nslab, ncell)
    for p in parts:
        assert (p.P, p.per) == (2, 1875) and p.nvec in (3750, 3749)
    assert M.batch_threads(1875) == 83 and M.remainder_threads(1875) == list(range(83, 256))
    assert M.batch_threads(3749 - 1875) == 82
    for tag in ('first', 'last'):
        for t in ('first', 'last'):
            assert set('%s block, first batch, %s thread, u%d' % (tag, t, u) for u in M.SLOTS) <= names
        assert '%s block, remainder, first vector' % tag in names
    assert set('head[%d]' % j for j in range(3)) | set('tail[%d]' % j for j in range(3)) <= names
    # no smaller launch gets there: a block needs more than 1792 vectors = 7168 float32 cells, which minmax_blocks allows only when the
    # fine rule (4096 cells a block) is cut by the 2048 blocks of the whole launch
    for ns, nc in ((1, 10 ** 6), (16, 10 ** 5), (350, 15001), (700, 14000)):
        P = M.minmax_blocks(nc, ns)
        assert -(-(nc // 4) // P) <= 1792, (ns, nc)


def test_more_partials_than_threads_in_the_final_reduction():
    nslab, ncell = M.MANY_BLOCKS
    for itemsize in (4, 8):
        parts, names = summary(itemsize, nslab, ncell)
        for p in parts:
            assert p.P == 301 and len(p.nonempty()) == 301 and max(M.FINAL_BLOCKS) == 300
        assert set('cut %d, %s' % (b, side) for b in range(1, 301) for side in ('before', 'after')) <= names
    assert nslab * ncell * 8 < 128 << 20


def test_schedule_deals_every_class_to_both_extrema():
    for itemsize in (4, 8):
        for nslab, ncell in M.SMALL + [M.ONE_BLOCK, M.SHORT_LAST, M.F32_UNROLLED]:
            for mis in M.misalignments(itemsize):
                per_slab = M.launch_classes(itemsize, ncell, nslab, mis)
                calls = M.schedule(per_slab)
                names = set(n for c in per_slab for n in c)
                for k in (0, 1):
                    assert set(pair[k] for call in calls for pair in call) - {None} == names
                for call in calls:
                    for c, (a, b) in zip(per_slab, call):
                        assert (a is None or a in c) and (b is None or b in c)
                        assert a is None or b is None or c[a] != c[b]
                if nslab == 700:
                    assert len(calls) == 1, 'one call covers all classes'
