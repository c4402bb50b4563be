"""The host half of find_contours, without a GPU: the restatement of K12's directed segments (contour_join_ref) against the
restatement of K10 (clength_ref), and xc_join_segments -- a host-only entry point of the library, through ctypes and in a
stand-alone program built with the address and undefined-behaviour sanitizers -- against the restatement's join."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import clength_ref as CR
import contour_join_ref as JR
from xcontour_amd import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = np.linspace(-2.0, 2.0, 7) + 0.0137


def plane(kind, ny=97, nx=301):
    rng = np.random.default_rng(11)
    if kind == 'saddle':
        return np.indices((ny, nx)).sum(0) % 2 * 2.0 - 1.0 + 0.3 * rng.standard_normal((ny, nx))       # checkerboard
    if kind == 'smooth':
        y, x = np.meshgrid(np.linspace(-1.5, 1.5, ny), np.linspace(0.0, 6.0, nx), indexing='ij')
        return 2.0 * np.sin(y) + 0.3 * np.cos(3 * x) * np.cos(y) ** 2 + 0.1 * np.sin(5 * x + 2 * y)
    q = rng.standard_normal((ny, nx))
    if kind == 'nan':
        q[rng.random(q.shape) < 0.03] = np.nan
    return q


KINDS = ['random', 'saddle', 'nan', 'smooth']


def rows(*cols):
    """a multiset of float64 rows as a sorted array of their bit patterns"""
    a = np.stack([np.ascontiguousarray(c, dtype=np.float64) for c in cols], axis=1).view(np.int64)
    return a[np.lexsort(a.T[::-1])]


@pytest.mark.parametrize('kind', KINDS)
def test_emission_equals_the_length_restatement(kind):
    q = plane(kind)
    for c, (ef, et, pts) in zip(LEVELS, JR.segments(q, LEVELS)):
        keep = ~((pts[:, 0] == pts[:, 2]) & (pts[:, 1] == pts[:, 3]))
        assert np.array_equal(rows(*pts[keep].T), rows(*CR.segments(q, c)))
        assert np.unique(ef).size == ef.size and np.unique(et).size == et.size
        assert ef.size > 0


def c_join(off, ef, et):
    """xc_join_segments through ctypes -> (rc, [[(segment indices relative to the range, closed), ...] per range])"""
    lib = nat.load()
    off, ef, et = (np.ascontiguousarray(a, dtype=np.int64) for a in (off, ef, et))
    total = ef.size
    order, poff = np.full(total, -7, dtype=np.int64), np.full(total + 1, -7, dtype=np.int64)
    closed, rpo = np.full(total, 9, dtype=np.uint8), np.full(off.size, -7, dtype=np.int64)
    rc = lib.xc_join_segments(off.size - 1, off.ctypes.data, ef.ctypes.data, et.ctypes.data, order.ctypes.data, poff.ctypes.data,
                              closed.ctypes.data, rpo.ctypes.data)
    if rc != 0:
        return rc, None
    out = []
    for r in range(off.size - 1):
        out.append([([int(i - off[r]) for i in order[poff[p]:poff[p + 1]]], bool(closed[p])) for p in range(rpo[r], rpo[r + 1])])
    assert sorted(order.tolist()) == list(range(total))
    return rc, out


def check_ranges(ranges):
    """`ranges`: [(e_from, e_to), ...] -> the library's join of all of them in one call == the restatement's, range by range"""
    off = np.concatenate([[0], np.cumsum([len(a) for a, _ in ranges])]).astype(np.int64)
    ef = np.concatenate([np.asarray(a, dtype=np.int64) for a, _ in ranges] + [np.zeros(0, dtype=np.int64)])
    et = np.concatenate([np.asarray(b, dtype=np.int64) for _, b in ranges] + [np.zeros(0, dtype=np.int64)])
    rc, got = c_join(off, ef, et)
    assert rc == 0
    assert got == [JR.join(a, b) for a, b in ranges]
    return got


@pytest.mark.parametrize('kind', KINDS)
def test_join_of_planes_equals_the_restatement(kind):
    rng = np.random.default_rng(5)
    ranges = []
    for ef, et, _ in JR.segments(plane(kind), LEVELS):
        o = rng.permutation(ef.size)                              # the C ABI promises no order inside a range
        ranges.append((ef[o], et[o]))
    got = check_ranges(ranges)
    assert any(not c for r in got for _, c in r)                                  # open polylines, and (the smooth plane has
    assert kind == 'smooth' or any(c for r in got for _, c in r)                  # none at these levels) rings


RING = ([10, 20, 30, 40], [20, 30, 40, 10])
CHAIN = ([5, 6, 7], [6, 7, 8])
MIXED = ([30, 5, 40, 6, 10, 7, 20], [40, 6, 10, 7, 20, 8, 30])       # RING and CHAIN interleaved in memory


def test_join_hand_made_cases():
    assert check_ranges([RING]) == [[([0, 1, 2, 3], True)]]
    assert check_ranges([CHAIN]) == [[([0, 1, 2], False)]]
    # the chain holds the smallest edge id: it comes first; the ring starts at its smallest e_from (10, at position 4)
    assert check_ranges([MIXED]) == [[([1, 3, 5], False), ([4, 6, 0, 2], True)]]
    got = check_ranges([RING, ([], []), CHAIN])
    assert got[1] == [] and got[0] == [([0, 1, 2, 3], True)] and got[2] == [([0, 1, 2], False)]
    rc, got = c_join([0], [], [])                                  # nrange = 0
    assert rc == 0 and got == []
    # a ring that does not begin at its smallest e_from in memory, two chains ordered by their smallest id (not by their head)
    assert check_ranges([([30, 10, 20], [10, 20, 30])]) == [[([1, 2, 0], True)]]
    assert check_ranges([([50, 3, 60, 1], [3, 4, 1, 2])]) == [[([2, 3], False), ([0, 1], False)]]


def test_join_rejects_malformed_input():
    rc, _ = c_join([0, 3], [5, 5, 7], [6, 7, 8])                 # duplicate e_from
    assert rc == nat.XC_EBADARG
    rc, _ = c_join([0, 4], [1, 2, 3, 4], [2, 3, 4, 2])           # duplicate e_to: 1 -> 2 -> 3 -> 4 -> 2 ..., a rho-shaped walk
    assert rc == nat.XC_EBADARG
    rc, _ = c_join([0, 2, 1], [1, 2], [2, 3])                    # descending offsets
    assert rc == nat.XC_EBADARG
    with pytest.raises(ValueError):
        JR.join([1, 2, 3, 4], [2, 3, 4, 2])
    with pytest.raises(nat.XContourHipError):
        nat.join_segments(np.array([0, 3]), np.array([5, 5, 7]), np.array([6, 7, 8]))


def test_nodes_exactly_on_the_level():
    rng = np.random.default_rng(3)
    q = rng.integers(0, 5, size=(40, 70)).astype(np.float64)
    (ef, et, pts), = JR.segments(q, [2.0])
    assert (pts[:, :2] == pts[:, 2:]).all(axis=1).any()            # coincident-end segments occur and are kept
    assert np.unique(ef).size == ef.size and np.unique(et).size == et.size       # degree 2: chains and rings only
    check_ranges([(ef, et)])
    # the pieces are those of the level one step up: there the same cells are crossed in the same cases, so the segments carry
    # the same edge ids and join into the same walks; a crossing that sits ON a node at 2.0 (frac 0) sits within 2^-52 / step
    # of it one step up, so what 2.0 merges into one vertex is, one step up, a run of vertices closer than 1e-12
    up = np.nextafter(2.0, np.inf)
    (ef2, et2, pts2), = JR.segments(q, [up])
    assert np.array_equal(ef, ef2) and np.array_equal(et, et2)
    assert np.abs(pts - pts2).max() <= 1e-12
    on, closed = JR.polylines(q, [2.0])
    assert len(on[0]) > 0 and True in closed[0] and False in closed[0]
    for v in on[0]:
        assert (v[1:] != v[:-1]).any(axis=1).all()                 # no consecutive duplicates
    near = []
    for segs, _ in JR.join(ef2, et2):
        v = np.concatenate([pts2[segs[:1], :2], pts2[segs, 2:]])
        keep = np.concatenate([[True], np.abs(v[1:] - v[:-1]).max(axis=1) > 1e-12])
        if keep.sum() >= 2:
            near.append(v[keep])
    assert len(near) == len(on[0])
    for a, b in zip(on[0], near):
        assert a.shape == b.shape and np.abs(a - b).max() <= 1e-12


MAIN = r'''
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "xcontour_hip.h"
static int run(int64_t nrange, const int64_t* off, const int64_t* ef, const int64_t* et, int want_rc, int64_t want_npoly)
{
    const int64_t total = off[nrange];
    int64_t* order = (int64_t*)malloc(sizeof(int64_t) * (size_t)(total ? total : 1));
    int64_t* poff = (int64_t*)malloc(sizeof(int64_t) * (size_t)(total + 1));
    uint8_t* closed = (uint8_t*)malloc((size_t)(total ? total : 1));
    int64_t* rpo = (int64_t*)malloc(sizeof(int64_t) * (size_t)(nrange + 1));
    const int rc = xc_join_segments(nrange, off, ef, et, order, poff, closed, rpo);
    int bad = rc != want_rc || (rc == 0 && (rpo[nrange] != want_npoly || poff[want_npoly] != total));
    if (bad) printf("case failed: rc %d (want %d)\n", rc, want_rc);
    free(order); free(poff); free(closed); free(rpo);
    return bad;
}
int main(void)
{
    int bad = 0;
    { const int64_t off[] = {0, 4}, ef[] = {10, 20, 30, 40}, et[] = {20, 30, 40, 10}; bad |= run(1, off, ef, et, 0, 1); }
    { const int64_t off[] = {0, 3}, ef[] = {5, 6, 7}, et[] = {6, 7, 8}; bad |= run(1, off, ef, et, 0, 1); }
    { const int64_t off[] = {0, 7}, ef[] = {30, 5, 40, 6, 10, 7, 20}, et[] = {40, 6, 10, 7, 20, 8, 30}; bad |= run(1, off, ef, et, 0, 2); }
    { const int64_t off[] = {0, 4, 4, 7}, ef[] = {10, 20, 30, 40, 5, 6, 7}, et[] = {20, 30, 40, 10, 6, 7, 8}; bad |= run(3, off, ef, et, 0, 2); }
    { const int64_t off[] = {0}; bad |= run(0, off, NULL, NULL, 0, 0); }
    { const int64_t off[] = {0, 3}, ef[] = {5, 5, 7}, et[] = {6, 7, 8}; bad |= run(1, off, ef, et, XC_EBADARG, 0); }
    { const int64_t off[] = {0, 4}, ef[] = {1, 2, 3, 4}, et[] = {2, 3, 4, 2}; bad |= run(1, off, ef, et, XC_EBADARG, 0); }
    puts(bad ? "FAILED" : "join ok");
    return bad;
}
'''


def test_join_stand_alone_under_sanitizers(tmp_path):
    """the join's translation unit and a small program of its own, built with g++ -fsanitize=address,undefined and run as a
    child process (never loaded into Python): the hand-made and the malformed cases"""
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('no g++')
    probe = tmp_path / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')

    def works(flags):
        return subprocess.run([gxx] + flags + ['-o', str(tmp_path / 'probe'), str(probe)], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT).returncode == 0 \
            and subprocess.run([str(tmp_path / 'probe')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).returncode == 0
    # the runtimes linked into the program itself where the static ones are installed: nothing about the run then depends on
    # which shared libraries the environment loads first
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan']
    if not works(san):
        san = san[:2]
        if not works(san):
            pytest.skip('the sanitizer runtime of g++ is not installed')
    main = tmp_path / 'join_main.cpp'
    main.write_text(MAIN)
    exe = str(tmp_path / 'join_main')
    subprocess.run([gxx, '-std=c++17', '-g', '-O1'] + san + ['-I', os.path.join(ROOT, 'include'), '-o', exe, str(main),
                    os.path.join(ROOT, 'xcontour_amd', 'csrc', 'xc_join.cpp')], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and 'join ok' in r.stdout, r.stdout
