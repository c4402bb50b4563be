"""xc_ring_tracks_dev (K23), the C entry on hand-built ring graphs, against cptrack_ref.tracks_of (a union-find in plain Python, not the
kernels' rounds): root, track, nprev, nnext, link_ok and every word of the track rows EQUAL.  No tolerances.  Every call hands the entry
arrays filled with a pattern, with guard elements before and behind each of them: on XC_OK exactly the outputs are written, otherwise
nothing but ntrack, and every guard is intact.

Rounds of the kernels on these cases, as measured: profiles/contour_piece_tracks.md; no bound on them is asserted here."""
import numpy as np
import pytest

import cptrack_ref as KR
from xcontour_amd import _native as nat

pytestmark = pytest.mark.gpu

GUARD = 16
I32, I64 = 0x5a5a5a5a, 0x5a5a5a5a5a5a5a5a
RING = (('root', np.int64), ('track', np.int64), ('nprev', np.int32), ('nnext', np.int32))
ROWS = tuple((k, KR.ROW_DTYPE[k].type) for k in KR.ROW_DTYPE.names)
CASES = KR.cases()


def pattern(n, t):
    return np.full(n + 2 * GUARD, 0x5a if t is np.uint8 else I32 if t is np.int32 else I64, dtype=t)


def call(ctx, c, capacity=None, mo=None, null_size=False):
    """one call -> (rc, ntrack or None, dict of the outputs as written or None); the guards are checked.  capacity None: what a count-only
    call asks for"""
    nring, nlink = c['nring'], c['la'].size
    mo = c['mo'] if mo is None else mo
    size = None if null_size else c['size']
    ins = [np.ascontiguousarray(c['step'], dtype=np.int32)] + ([np.ascontiguousarray(size, dtype=np.int64)] if size is not None else [])
    ins += [np.ascontiguousarray(c[k], dtype=np.int64) for k in ('la', 'lb', 'ln')] if nlink else []
    if capacity is None:
        rc, nt, _ = call(ctx, c, capacity=0, mo=mo, null_size=null_size)
        assert rc == 1 and nt >= 1, 'the count-only call returned %d' % rc
        capacity = nt
    ncap = max(capacity, 1)
    outs = [pattern(nring, t) for _, t in RING] + [pattern(max(nlink, 1), np.uint8), pattern(1, np.uint64)] + [pattern(ncap, t) for _, t in ROWS]
    with ctx._temporaries(ins + outs, []) as bufs:
        d_in, d_out = bufs[:len(ins)], bufs[len(ins):]
        dl = [b.ptr for b in d_in[-3:]] if nlink else [None] * 3
        at = [b.ptr + GUARD * a.dtype.itemsize for b, a in zip(d_out, outs)]
        if capacity == 0:
            at = [None] * 5 + [at[5]] + [None] * 6
        rc = ctx.lib.xc_ring_tracks_dev(ctx.handle, nring, nlink, d_in[0].ptr, d_in[1].ptr if size is not None else None, *dl, float(mo),
                                        *at[:5], capacity, *at[5:])
        back = [b.download(a.shape, a.dtype) for b, a in zip(d_out, outs)]
    nt = None if back[5][GUARD] == I64 else int(back[5][GUARD])
    wrote = rc == 0
    sizes = [nring] * 4 + [nlink, 1] + [nt if wrote else 0] * 6
    got = {}
    for (name, _), b, a, n in zip(RING + (('link_ok', 0), ('ntrack', 0)) + ROWS, back, outs, sizes):
        keep = n if (wrote or name == 'ntrack') else 0
        if name == 'ntrack' and nt is None:
            keep = 0
        assert b[:GUARD].tobytes() == a[:GUARD].tobytes(), 'the guard before %s was written' % name
        assert b[GUARD + keep:].tobytes() == a[GUARD + keep:].tobytes(), '%s was written behind its %d words' % (name, keep)
        got[name] = b[GUARD:GUARD + keep]
    if not wrote:
        return rc, nt, None
    rows = np.empty(nt, dtype=KR.ROW_DTYPE)
    for k, _ in ROWS:
        rows[k] = got[k]
    return rc, nt, dict(root=got['root'], track=got['track'], nprev=got['nprev'], nnext=got['nnext'], link_ok=got['link_ok'].astype(bool), rows=rows)


def reference(c, **kw):
    a = dict(c, **kw)
    return KR.tracks_of(a['nring'], a['step'], a['size'], a['la'], a['lb'], a['ln'], a['mo'])


@pytest.fixture(scope='module')
def refs():
    return {name: reference(c) for name, c in CASES.items()}                  # computed once, shared, never changed


@pytest.mark.parametrize('name', list(CASES))
def test_every_hand_built_graph(ctx, refs, name):
    c, ref = CASES[name], refs[name]
    rc, nt, got = call(ctx, c)
    assert rc == 0 and nt == ref['rows'].size
    assert KR.same(got, ref), name
    prof = ctx.last_cptrack_profile()
    assert prof['rounds'] >= (2 if ref['link_ok'].any() else 1 if c['la'].size else 0)      # a last round changes nothing
    print('%s: %d rounds' % (name, prof['rounds']))
    if name == 'diamond':
        assert got['rows'].tolist() == [(0, 0, 2, 4, 1, 1), (4, 2, 2, 1, 0, 0)]
    if name == 'two chains that meet at their last rings':
        assert (got['root'] == 0).all()
    if name == 'one ring, no link':
        assert got['rows'].tolist() == [(0, 0, 0, 1, 0, 0)] and prof['rounds'] == 0


def test_the_chain_gives_the_same_words_in_every_link_order(ctx):
    outs = [call(ctx, CASES['chain of 5000, %s' % order])[2] for order in ('ascending', 'reversed', 'shuffled')]
    for o in outs[1:]:
        assert all(o[k].tobytes() == outs[0][k].tobytes() for k in ('root', 'track', 'nprev', 'nnext', 'rows'))
    assert (outs[0]['root'] == 0).all() and outs[0]['rows'].tolist() == [(0, 0, 4999, 5000, 0, 0)]


def test_ring_size_null_with_min_overlap_0_and_its_refusal_otherwise(ctx, refs):
    c = CASES['255 rings, 255 links']                                        # it has sizes and min_overlap 0
    assert c['size'] is not None and c['mo'] == 0.0
    rc, _, got = call(ctx, c, null_size=True)
    assert rc == 0 and KR.same(got, refs['255 rings, 255 links'])
    rc, nt, got = call(ctx, c, capacity=c['nring'], mo=0.5, null_size=True)
    assert rc == nat.XC_EBADARG and nt is None and got is None
    rc, _, got = call(ctx, c, mo=0.5)                                         # the same graph with its sizes and a threshold
    assert rc == 0 and KR.same(got, reference(c, mo=0.5)) and not KR.same(got, refs['255 rings, 255 links'])


def test_capacity_one_short_writes_the_count_alone(ctx, refs):
    c, ref = CASES['257 rings, 257 links'], refs['257 rings, 257 links']
    nt = ref['rows'].size
    assert nt > 1
    rc, got_nt, got = call(ctx, c, capacity=nt - 1)
    assert rc == 1 and got_nt == nt and got is None
    rc, got_nt, got = call(ctx, c, capacity=nt + 5)
    assert rc == 0 and got_nt == nt and KR.same(got, ref)


def test_refusals_write_nothing(ctx):
    c = CASES['diamond']
    for key, at, v in (('la', 1, 5), ('lb', 3, 5), ('lb', 0, 1 << 40)):                   # a ring >= nring, on either side
        bad = dict(c, **{key: c[key].copy()})
        bad[key][at] = v
        rc, nt, got = call(ctx, bad, capacity=5)
        assert rc == nat.XC_EBADARG and nt is None and got is None, (key, v)
        assert b'nring' in ctx.lib.xc_last_error(ctx.handle)
    for mo in (np.nan, -0.25, 1.5, np.inf):
        rc, nt, got = call(ctx, dict(c, size=np.ones(5, dtype=np.int64)), capacity=5, mo=mo)
        assert rc == nat.XC_EBADARG and nt is None and got is None, mo
    rc, _, got = call(ctx, c)                                                 # and the context still works
    assert rc == 0 and got['root'].tolist() == [0, 0, 0, 0, 4]
