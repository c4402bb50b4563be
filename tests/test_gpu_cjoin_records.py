"""xc_contour_polylines_dev (K14) on records the TEST built (builders of cpiece_records_ref), against the host join xc_join_segments:
the walk order, the polyline table and the gathered records, all integers or bit patterns, all equal.  The sizes sit where a doubling
count or a scan chunk can be off by one.  Every output buffer of every call carries guard elements past its end, filled with a
sentinel, and they are checked after every call."""
import functools

import numpy as np
import pytest

import cpiece_records_ref as RR
from xcontour_amd import _native as nat

pytestmark = pytest.mark.gpu

NY, NX = 8, 300                         # E = 4800 edge ids: no multiple of the scan chunk
E = 2 * NY * NX
CHUNK = 2048                            # CJ_CHUNK of xc_cjoin.hip: table entries per block of the placement scan
DEFAULT_CAP = 1 << 30
GUARD = 8                               # elements past the end of every output buffer
S64, S32, SF = -0x0123456789abcdef, -0x01234567, -1.25e300


def call_dev(ctx, count, e_from, e_to, pts, ny=NY, nx=NX, capacity=None, arrays=True):
    """one xc_contour_polylines_dev call on host records -> (rc, dict of the seven output buffers as the entry left them, guards
    included, every element preset to a sentinel).  capacity: default the number of segments; arrays=False: NULL arrays."""
    count = np.ascontiguousarray(count, dtype=np.uint64).ravel()
    total, nr = int(count.sum()), count.size
    cap = total if capacity is None else capacity
    ins = [count, np.ascontiguousarray(e_from, dtype=np.int64), np.ascontiguousarray(e_to, dtype=np.int64),
           np.ascontiguousarray(pts, dtype=np.float64).reshape(-1)]
    ins = [a if a.size else np.zeros(1, dtype=a.dtype) for a in ins]
    outs = dict(poly_count=np.full(nr + GUARD, S64, dtype=np.int64), nseg=np.full(cap + GUARD, S64, dtype=np.int64),
                closed=np.full(cap + GUARD, S32, dtype=np.int32), first=np.full(cap + GUARD, S64, dtype=np.int64),
                pts_walk=np.full(4 * total + GUARD, SF, dtype=np.float64), ef_walk=np.full(total + GUARD, S64, dtype=np.int64),
                order=np.full(total + GUARD, S64, dtype=np.int64))
    with ctx._temporaries(ins + list(outs.values()), []) as (dn, df, dt, dp, *dev):
        ptr = {k: b.ptr for k, b in zip(outs, dev)}
        null = lambda k: ptr[k] if arrays else None
        rc = ctx.lib.xc_contour_polylines_dev(ctx.handle, nr, dn.ptr, df.ptr, dt.ptr, dp.ptr, ny, nx, cap, ptr['poly_count'],
                                              null('nseg'), null('closed'), null('first'), null('pts_walk'), null('ef_walk'), null('order'))
        got = {k: b.download(outs[k].shape, outs[k].dtype) for k, b in zip(outs, dev)}
    used = dict(poly_count=nr, nseg=cap, closed=cap, first=cap, pts_walk=4 * total, ef_walk=total, order=total)
    for k, v in got.items():
        assert (v[used[k]:] == outs[k][0]).all(), 'the guard elements behind %s were written' % k
    return rc, got


def untouched(got, *but):
    for k, v in got.items():
        if k not in but:
            assert (v == {'closed': S32, 'pts_walk': SF}.get(k, S64)).all(), '%s was written' % k


def host_join(count, e_from, e_to, pts):
    count = np.asarray(count).astype(np.int64).ravel()
    off = np.concatenate([[0], np.cumsum(count)])
    order, poff, closed, rpo = nat.join_segments(off, e_from, e_to)
    ef = np.asarray(e_from, dtype=np.int64)[order]
    first = np.minimum.reduceat(ef, poff[:-1]) if poff.size > 1 else np.zeros(0, dtype=np.int64)
    return dict(poly_count=np.diff(rpo), nseg=np.diff(poff), closed=closed.astype(np.int32), first=first,
                pts_walk=np.asarray(pts, dtype=np.float64).reshape(-1, 4)[order].reshape(-1), ef_walk=ef, order=order)


def check(ctx, count, e_from, e_to, pts, what='', cap=None, **plane):
    """the entry against the host join, everything equal (pts bit for bit) -> the entry's outputs, cut to size"""
    try:
        if cap is not None:
            ctx.set_cpiece_workspace(cap)
        rc, got = call_dev(ctx, count, e_from, e_to, pts, **plane)
    finally:
        if cap is not None:
            ctx.set_cpiece_workspace(DEFAULT_CAP)
    assert rc == 0, '%s: xc_contour_polylines_dev returned %d' % (what, rc)
    ref = host_join(count, e_from, e_to, pts)
    out = {}
    for k, r in ref.items():
        g = got[k][:r.size]
        same = np.array_equal(g.view(np.int64), r.view(np.int64)) if r.dtype == np.float64 else np.array_equal(g, r)
        assert same, '%s: %s differs from the host join (first at %d)' % (what, k, int(np.flatnonzero(g != r)[0]) if g.size else -1)
        out[k] = g
    return out


# ------------------------------------------------------------------ chains of every length, order and place of the smallest id
@functools.lru_cache(maxsize=None)
def chains(closed):
    return RR.one_chain_per_range(closed, NY, NX)


@pytest.mark.parametrize('cap', [None, 1], ids=['default cap', 'one range per group'])
@pytest.mark.parametrize('closed', [True, False], ids=['rings', 'open chains'])
def test_one_chain_per_range_every_length_order_and_place_of_the_smallest_id(ctx, closed, cap):
    """chains of 1 .. 4097 segments (1, 2, 3, 63, 64, 65, 4096, 4097 among them; a ring from 2) stored forward, reversed, strided
    and shuffled, the smallest id at the head, the middle and the tail.  A ring must start AT its smallest id, an open chain at
    its head wherever the smallest id is.  One range per group gives every length the round count of its own size."""
    cnt, ef, et, pts, expect = chains(closed)
    assert {1, 2, 3, 63, 64, 65, 4096, 4097} - {n for _, n in expect} == ({1} if closed else set())
    out = check(ctx, cnt, ef, et, pts, 'chains', cap=cap)
    assert np.array_equal(out['poly_count'], np.ones(cnt.size)) and np.array_equal(out['nseg'], [n for _, n in expect])
    assert np.array_equal(out['first'], [f for f, _ in expect]) and (out['closed'] == int(closed)).all()
    if closed:
        heads = np.concatenate([[0], np.cumsum(out['nseg'])[:-1]])
        assert np.array_equal(out['ef_walk'][heads], out['first'])


# ------------------------------------------------------------------ many pieces across the scan's chunk boundaries
def straddling_pieces(seed=12):
    """450 pieces in one range.  Roots (smallest ids) on the last entry of a scan chunk and on the first entry of the next, on id
    0 and on the table's last id: E = 4800 is 2 chunks of 2048 and a part of one."""
    rng = np.random.default_rng(seed)
    special = [CHUNK - 1, 3000, CHUNK, 3001, 2 * CHUNK - 1, 4500, 2 * CHUNK, 4501, 0, 4700]
    sizes = [(2, True)] * 5 + [(1, False)] + [(2, True)] * 295 + [(1, False)] * 99 + [(int(n), False) for n in rng.integers(3, 10, 50)]
    rest = rng.permutation(np.setdiff1d(np.arange(E - 1), special))
    nid = sum(n for n, _ in sizes)
    ids = np.concatenate([special, [E - 1], rest])
    ef, et, pts = RR.pieces_of_sizes(sizes, ids[:nid], ids[nid:nid + 150], rng, NY, NX)
    return np.array([ef.size], dtype=np.uint64), ef, et, pts


def test_450_pieces_whose_roots_straddle_the_scan_chunks(ctx):
    assert E % CHUNK != 0 and E > 2 * CHUNK
    cnt, ef, et, pts = straddling_pieces()
    out = check(ctx, cnt, ef, et, pts, 'straddling')
    assert out['poly_count'][0] == 450
    first = out['first'].tolist()
    assert first == sorted(first) and first[0] == 0 and first[-1] == E - 1
    for edge in (CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK):
        assert edge in first
    k = first.index(CHUNK - 1)
    assert first[k + 1] == CHUNK                                             # neighbours in the table, in two chunks


def test_many_pieces_of_the_k13_case(ctx):
    cnt, ef, et, pts, npiece = RR.many_pieces(NY, NX)
    assert check(ctx, cnt, ef, et, pts, 'many pieces')['poly_count'][0] == npiece == 450


# ------------------------------------------------------------------ ranges that share ids, groups, waves across ranges
SHORT = [0, 1, 0, 63, 64, 65, 0, 130, 1, 0, 2, 0]


@pytest.mark.parametrize('counts', [SHORT, [2, 4097, 0, 2], [40, 24]],
                         ids=['short ranges', 'a long range beside short ones', 'one wave over two ranges'])
def test_ranges_that_share_their_edge_ids_under_three_workspace_caps(ctx, counts):
    """every range draws the SAME edge ids; waves and blocks straddle range boundaries ([40, 24]: one wave of 64 lanes holds both
    ranges); empty ranges in front, between and behind.  The cap moves the group boundaries and nothing else: a group of one
    range, of three ranges, of all."""
    rec = RR.short_ranges(counts, NY, NX)
    outs = [check(ctx, *rec, what='cap %r' % (cap,), cap=cap) for cap in (None, 1, 3 * E * 4)]
    for o in outs[1:]:
        for k in o:
            assert np.array_equal(o[k], outs[0][k]), k
    assert np.array_equal(outs[0]['poly_count'] > 0, np.asarray(counts) > 0)


# ------------------------------------------------------------------ K12's own records in any storage order
def test_k12_records_permuted_inside_every_range_give_the_same_polylines(ctx):
    rng = np.random.default_rng(23)
    q = rng.standard_normal((97, 301))
    q[rng.random(q.shape) < 0.03] = np.nan
    lv = np.concatenate([[-9.0], np.linspace(-2.0, 2.0, 8), [11.0, np.inf]])
    cnt, ef, et, pts = ctx.contour_segments(q[None], lv)
    plane = dict(ny=97, nx=301)
    base = check(ctx, cnt.ravel(), ef, et, pts, 'K12 order', **plane)
    assert base['poly_count'].sum() > 2000 and base['poly_count'][0] == 0 and base['poly_count'][-1] == 0
    off = np.concatenate([[0], np.cumsum(cnt.ravel().astype(np.int64))])
    for how in ('reversed', 'random'):
        o = np.concatenate([a + (np.arange(b - a)[::-1] if how == 'reversed' else rng.permutation(b - a)) for a, b in zip(off[:-1], off[1:])])
        got = check(ctx, cnt.ravel(), ef[o], et[o], pts[o], how, **plane)
        for k in ('poly_count', 'nseg', 'closed', 'first', 'ef_walk'):
            assert np.array_equal(got[k], base[k]), (how, k)
        assert np.array_equal(got['pts_walk'].view(np.int64), base['pts_walk'].view(np.int64)), how
        assert np.array_equal(o[got['order']], base['order']), how


# ------------------------------------------------------------------ malformed records
def malformed(which):
    cnt, ef, et, pts, _ = RR.many_pieces(NY, NX)
    ef, et = ef.copy(), et.copy()
    if which == 'a repeated e_from':
        ef[517] = ef[3]
    elif which == 'a repeated e_to that has a successor':
        i = int(np.flatnonzero(np.isin(et, ef))[5])
        j = int(np.flatnonzero(np.isin(et, ef))[40])
        et[j] = et[i]
    elif which == 'a repeated e_to without successor':
        t = np.flatnonzero(~np.isin(et, ef))
        et[int(t[7])] = et[int(t[3])]
    elif which == 'e_from past the table':
        ef[517] = E
    elif which == 'a negative e_to':
        et[517] = -1
    return cnt, ef, et, pts


@pytest.mark.parametrize('which', ['a repeated e_from', 'a repeated e_to that has a successor', 'a repeated e_to without successor',
                                   'e_from past the table', 'a negative e_to'])
def test_malformed_records_are_refused_and_the_next_call_is_right(ctx, which):
    """XC_EBADARG, as from the host join; nothing but poly_count is written (the guards are checked inside call_dev); the edge
    table is handed on clean: the same context joins valid records right afterwards"""
    cnt, ef, et, pts = malformed(which)
    if 'repeated' in which:
        off = np.array([0, ef.size], dtype=np.int64)
        with pytest.raises(nat.XContourHipError):
            nat.join_segments(off, ef, et)                                   # the host join's rule
    rc, got = call_dev(ctx, cnt, ef, et, pts)
    assert rc == nat.XC_EBADARG, which
    untouched(got, 'poly_count')
    good = RR.many_pieces(NY, NX)[:4]
    check(ctx, *good, what='the call after the refused one')
    rec = RR.short_ranges(SHORT, NY, NX)
    check(ctx, *rec, what='the second call after the refused one')


# ------------------------------------------------------------------ the capacity protocol
def test_count_only_and_a_capacity_one_short_write_the_counts_alone(ctx):
    rec = RR.short_ranges(SHORT, NY, NX)
    ref = host_join(*rec)
    npoly = int(ref['poly_count'].sum())
    rc, got = call_dev(ctx, *rec, capacity=0, arrays=False)
    assert rc == 1 and np.array_equal(got['poly_count'][:len(SHORT)], ref['poly_count'])
    untouched(got, 'poly_count')
    rc, got = call_dev(ctx, *rec, capacity=npoly - 1)
    assert rc == 1 and np.array_equal(got['poly_count'][:len(SHORT)], ref['poly_count'])
    untouched(got, 'poly_count')
    rc, got = call_dev(ctx, *rec, capacity=npoly)
    assert rc == 0
    for k, r in ref.items():
        assert np.array_equal(got[k][:r.size].view(np.int64), r.view(np.int64)) if r.dtype == np.float64 else np.array_equal(got[k][:r.size], r), k


def test_no_segments_at_all(ctx):
    z = np.zeros(0)
    for arrays in (True, False):
        rc, got = call_dev(ctx, [0, 0, 0], z, z, z, capacity=0, arrays=arrays)
        assert rc == 0 and (got['poly_count'][:3] == 0).all()
        untouched(got, 'poly_count')
