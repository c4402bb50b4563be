"""xc_ring_tracks_dev (K23) where its launch geometry and its atomics can fail, against cptrack_ref.tracks_of (a union-find in plain
Python) and, for the two graphs of 2^24 + 300 rings, the closed forms of cptrack_geometry_cases.py: root, track, nprev, nnext, link_ok and
every word of the track rows EQUAL, no tolerances.  The graphs are cptrack_geometry_cases' (test_cptrack_geometry_host.py shows on the CPU
that each has what its tag names): steps in any order and over all of int32, links with a > b and a == b, a chain of many rounds, rings
of degree 93 332, roots on both sides of a wave and a block, calls without links and with every link rejected, the conversions of the
accept rule, a second trip of every grid-stride loop.  The calls go through the guarded-output `call` of test_gpu_cptrack_records.py:
patterns and guards behind every array, exactly the outputs written on XC_OK and nothing on a refusal.

Of the rounds only what the header fixes is asserted (cptrack_geometry_cases.rounds_fixed): 0 without links, 1 when no accepted link
joins two different rings, otherwise at least 2 and at most nring + 1; the measured ones are printed and stand in
profiles/contour_piece_tracks.md."""
import time

import numpy as np
import pytest

import cpoverlap_ref as OR
import cptrack_geometry_cases as GC
import cptrack_ref as KR
import test_gpu_cpoverlap_records as T22
import test_gpu_cptrack_records as T23
from xcontour_amd import _native as nat

pytestmark = pytest.mark.gpu

CASES = GC.cases()
WORDS = ('root', 'track', 'nprev', 'nnext', 'rows')


@pytest.fixture(scope='module')
def refs():
    return {name: GC.reference(c) for name, c in CASES.items()}              # computed once, shared, never changed


def check_rounds(ctx, c, ref, what):
    rounds = ctx.last_cptrack_profile()['rounds']
    print('%s: %d rounds' % (what, rounds))
    fixed = GC.rounds_fixed(c, ref)
    assert rounds == fixed if fixed is not None else 2 <= rounds <= c['nring'] + 1, (what, rounds)


def same_words(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in WORDS)


@pytest.mark.parametrize('name', list(CASES))
def test_every_graph_of_the_geometry(ctx, refs, name):
    c, ref = CASES[name], refs[name]
    rc, nt, got = T23.call(ctx, c)
    assert rc == 0 and nt == ref['rows'].size
    assert KR.same(got, ref), name
    check_rounds(ctx, c, ref, name)
    for key, v in c['want'].items():                                         # the answers written out
        if key == 'rows':
            assert got['rows'].tolist() == v
        elif key == 'first_ring':
            assert got['rows']['first_ring'].tolist() == v
        else:
            assert got[key].tolist() == v, key
    if c['group'] == 'hub':
        side = name[-1]
        hub = int(c['l' + side][0])
        assert got['nnext' if side == 'a' else 'nprev'][hub] == c['la'].size
        assert got['rows'][0]['nsplit' if side == 'a' else 'nmerge'] == 1 and nt == 1
    if c['group'] not in ('direction', 'hub'):
        return
    d, p = GC.shuffled(c)                                                    # any link order: the same words
    rc, _, again = T23.call(ctx, d)
    assert rc == 0 and same_words(again, got) and np.array_equal(again['link_ok'], got['link_ok'][p])


@pytest.mark.parametrize('name', list(GC.refusals()))
def test_a_ring_index_beyond_nring_is_refused_and_nothing_is_written(ctx, refs, name):
    case, at, link = GC.refusals()[name]
    c = CASES[case]
    rc, nt, got = T23.call(ctx, GC.with_link(c, at, link), capacity=c['nring'])
    assert rc == nat.XC_EBADARG and nt is None and got is None, name
    assert b'nring' in ctx.lib.xc_last_error(ctx.handle)
    rc, _, got = T23.call(ctx, c)                                             # and the context still works
    assert rc == 0 and KR.same(got, refs[case])


def test_the_shared_workspaces_keep_nothing_from_a_larger_call_or_from_k22(ctx, refs):
    old = T23.CASES
    seq = [('hub 69999 of 70 000 as b', CASES), ('diamond', old), ('257 rings, 257 links', old)]
    first = {}
    for name, cases in seq:
        rc, _, got = T23.call(ctx, cases[name])
        assert rc == 0, name
        first[name] = got
    assert KR.same(first['hub 69999 of 70 000 as b'], refs['hub 69999 of 70 000 as b'])
    for name in ('diamond', '257 rings, 257 links'):
        assert KR.same(first[name], T23.reference(old[name])), '%s after the hub' % name
    la, lb, w, f = OR.cases()['blobs']                                       # K22 lays its tables out in the same two blocks
    rc, pc, _ = T22.call(ctx, la[None], lb[None], 1, w, f[None])
    assert rc == 0 and pc.sum() > 0
    rc, _, got = T23.call(ctx, old['diamond'])
    assert rc == 0 and same_words(got, first['diamond']) and np.array_equal(got['link_ok'], first['diamond']['link_ok'])
    assert got['rows'].tolist() == [(0, 0, 2, 4, 1, 1), (4, 2, 2, 1, 0, 0)]
    for name, cases in seq:                                                  # and once more round: every call gives its first words
        rc, _, got = T23.call(ctx, cases[name])
        assert rc == 0 and same_words(got, first[name]) and np.array_equal(got['link_ok'], first[name]['link_ok']), name


# ------------------------------------------------------------------ 2^24 + 300 rings and links: RT_MAX_BLOCKS * RT_TPB and a second trip
def count_only(ctx, c):
    """a call with capacity 0 and no output but ntrack -> (rc, ntrack)"""
    ins = [np.ascontiguousarray(c['step'], dtype=np.int32)] + [np.ascontiguousarray(c[k], dtype=np.int64) for k in ('la', 'lb', 'ln')]
    with ctx._temporaries(ins + [np.zeros(1, dtype=np.uint64)], []) as bufs:
        rc = ctx.lib.xc_ring_tracks_dev(ctx.handle, c['nring'], c['la'].size, bufs[0].ptr, None, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr,
                                        float(c['mo']), *[None] * 5, 0, bufs[4].ptr, *[None] * 6)
        return rc, int(bufs[4].download((1,), np.uint64)[0])


def large(ctx, g, closed, what):
    t0 = time.perf_counter()
    rc, nt, got = T23.call(ctx, g, capacity=closed['rows'].size)             # the capacity is known: no count-only call
    t1 = time.perf_counter()
    assert rc == 0 and nt == closed['rows'].size
    for k in ('root', 'track', 'nprev', 'nnext', 'link_ok'):
        assert np.array_equal(got[k], closed[k]), (what, k)
    for k in KR.ROW_DTYPE.names:
        assert np.array_equal(got['rows'][k], closed['rows'][k]), (what, k)
    check_rounds(ctx, g, closed, what)
    print('%s: the guarded call %.2f s, the comparison %.2f s' % (what, t1 - t0, time.perf_counter() - t1))


def test_the_second_trip_of_the_grid_stride_loops_on_pairs(ctx):
    t0 = time.perf_counter()
    g, closed = GC.second_trip()
    assert g['nring'] == g['la'].size == GC.RT_MAX_BLOCKS * GC.RT_TPB + GC.TAIL
    print('pairs: the graph and its closed form %.2f s' % (time.perf_counter() - t0))
    large(ctx, g, closed, 'pairs, %d rings and links' % g['nring'])


def test_the_second_trip_alone_joins_flattens_and_counts_the_last_300_rings(ctx):
    """the last 300 rings are one track through links of the second trip alone.  Before it a count-only call on a graph of the same sizes
    leaves ring 0 as the parent of those 300 rings in the workspace, so an init that skipped them would show as root 0."""
    poison = GC.tail_poison()
    rc, nt = count_only(ctx, poison)
    assert rc == 1 and nt == poison['nring'] - GC.TAIL
    g, closed = GC.second_trip_chained()
    assert g['nring'] == poison['nring'] and g['la'].size == poison['la'].size
    large(ctx, g, closed, 'chained tail, %d rings and links' % g['nring'])
    assert (closed['root'][GC.STRIDE:] == GC.STRIDE).all() and closed['rows'][-1]['nrings'] == GC.TAIL
