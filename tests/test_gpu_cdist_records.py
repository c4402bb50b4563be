"""xc_contour_distance_dev (K27), the C entry on records the TEST built (cdist_cases), against cdist_ref: on the plane dist BIT FOR BIT,
edge and piece equal.  test_cdist_host.py shows on the CPU that the restatement tells a wrong rule on these inputs.  Every call hands
the entry outputs filled with a pattern and followed by guard elements: on XC_OK every element is written and every guard intact, on
a refusal nothing is touched."""
import numpy as np
import pytest

import cdist_cases as CC
import cdist_ref as DR
from xcontour_amd import _native as nat

pytestmark = pytest.mark.gpu

GUARD = 16
PATTERN = {np.float64: -1.2345e300, np.int64: 0x5a5a5a5a5a5a5a5a}
TYPES = (np.float64, np.int64, np.int64)
NAMES = ('dist', 'edge', 'piece')


def call(ctx, c, select=0, max_dist=0.0, mask=None, period=None, prune=True, cap=None):
    """one call -> (rc, dict(dist, edge, piece), untouched)"""
    cnt, ef, et, pts = c['rec']
    cnt = np.ascontiguousarray(cnt, dtype=np.uint64).ravel()
    nr, ny, nx = cnt.size, c['ny'], c['nx']
    n = nr * ny * nx
    ins = [cnt, np.ascontiguousarray(ef, dtype=np.int64), np.ascontiguousarray(et, dtype=np.int64), np.ascontiguousarray(pts, dtype=np.float64).ravel(),
           np.ascontiguousarray(c['ycoord'], dtype=np.float64), np.ascontiguousarray(c['xcoord'], dtype=np.float64)]
    ins = [a if a.size else np.zeros(1, dtype=a.dtype) for a in ins]
    if mask is not None:
        ins.append(np.ascontiguousarray(mask, dtype=np.uint8).ravel())
    outs = [np.full(n + GUARD, PATTERN[t], dtype=t) for t in TYPES]
    try:
        ctx.set_cdist_prune(prune)
        if cap is not None:
            ctx.set_cpiece_workspace(cap)
        with ctx._temporaries(ins + outs, []) as bufs:
            dm = bufs[6].ptr if mask is not None else None
            dout = bufs[-3:]
            rc = ctx.lib.xc_contour_distance_dev(ctx.handle, nr, *[b.ptr for b in bufs[:4]], ny, nx, c['periodic'], int(select), bufs[4].ptr,
                                                 bufs[5].ptr, c['period'] if period is None else period, c['radius'], float(max_dist), dm,
                                                 *[b.ptr for b in dout])
            back = [b.download((n + GUARD,), t) for b, t in zip(dout, TYPES)]
    finally:
        ctx.set_cdist_prune(True)
        if cap is not None:
            ctx.set_cpiece_workspace(1 << 30)
    pat = [np.full(n + GUARD, PATTERN[t], dtype=t).view(np.int64) for t in TYPES]
    for name, b, p in zip(NAMES, back, pat):
        assert (b.view(np.int64)[n:] == p[n:]).all(), 'the guard behind %s was written' % name
    untouched = all((b.view(np.int64)[:n] == p[:n]).all() for b, p in zip(back, pat))
    return rc, {name: b[:n].reshape(nr, ny, nx) for name, b in zip(NAMES, back)}, untouched


def same(got, ref, what):
    assert DR.same_bits(got['dist'], ref['dist']), '%s: dist differs at %d nodes' % (
        what, int((got['dist'].view(np.int64) != ref['dist'].view(np.int64)).sum()))
    assert np.array_equal(got['edge'], ref['edge']), '%s: edge' % what
    assert np.array_equal(got['piece'], ref['piece']), '%s: piece' % what


def run(ctx, c, what, select=0, **kw):
    rc, got, _ = call(ctx, c, select, **kw)
    assert rc == 0, '%s: xc_contour_distance_dev returned %d' % (what, rc)
    return got


@pytest.mark.parametrize('name', sorted(CC.plane_cases()))
def test_planes_around_a_tile_and_blocks_of_every_chunk_count(ctx, name):
    """16 x 16, 17 x 33, 37 x 45 and two rows; a range without segments (+inf, -1); smooth levels and white noise, whose blocks take
    more than one LDS chunk; pruned, unpruned and one range per group give the same bits"""
    c = CC.plane_cases()[name]
    ref = CC.reference(c)
    got = run(ctx, c, name)
    same(got, ref, name)
    empty = np.flatnonzero(c['rec'][0].ravel() == 0)
    for r in empty:
        assert np.isposinf(got['dist'][r]).all() and (got['edge'][r] == -1).all() and (got['piece'][r] == -1).all()
    for kw in (dict(prune=False), dict(cap=1)):
        again = run(ctx, c, name, **kw)
        same(again, got, '%s %r' % (name, kw))


def test_noise_blocks_take_more_than_one_chunk():
    """the white-noise cases put more than 256 segments into one 32 x 32 block of cells"""
    for name in ('37x45 noise', '37x40 ring noise'):
        c = CC.plane_cases()[name]
        n0 = int(c['rec'][0].ravel()[0])
        node = np.asarray(c['rec'][1][:n0]) >> 1
        bid = (node // c['nx'] // DR.BLOCK) * 8 + (node % c['nx']) // DR.BLOCK
        assert np.bincount(bid).max() > 256


def test_diamond_ties_and_exact_values(ctx):
    c = CC.diamond_case()
    got = run(ctx, c, 'diamond')
    same(got, CC.reference(c), 'diamond')
    assert got['dist'][0, 8, 8] == np.sqrt(8.0) and got['edge'][0, 8, 8] == c['rec'][1][:4].min()


@pytest.mark.parametrize('select', [0, 1, 2])
def test_every_select_on_the_ring(ctx, select):
    """a wavy circumpolar ring, a shorter one and a blob on a periodic 37 x 40 plane: image shifts and K16's selection"""
    c = CC.ring_case()
    ref = CC.reference(c, select)
    got = run(ctx, c, 'ring', select)
    same(got, ref, 'ring select %d' % select)
    if select == 2:
        assert len(np.unique(got['piece'][0])) == 1 and len(np.unique(CC.reference(c, 1)['piece'][0])) == 2
    same(run(ctx, CC.shuffled(c), 'ring shuffled', select), got, 'shuffled records')
    same(run(ctx, c, 'ring unpruned', select, prune=False), got, 'unpruned')


def test_cap_and_negate_mask(ctx):
    c = CC.ring_case()
    ref = CC.reference(c)
    d = ref['dist'][np.isfinite(ref['dist'])]
    cap = float(0.5 * (d.min() + d.max()))
    mask = (np.random.default_rng(2).random(ref['dist'].shape) < 0.5).astype(np.uint8)
    refc = CC.reference(c, max_dist=cap, negate_mask=mask)
    assert np.isinf(refc['dist']).any() and (refc['dist'] < 0).any()
    for prune in (True, False):
        same(run(ctx, c, 'cap', max_dist=cap, mask=mask, prune=prune), refc, 'cap + mask, prune %r' % prune)


def test_sphere_records(ctx):
    """the sphere's metric on records: within the bound the facade test derives, and the returned segment is (one of) the nearest"""
    R = 6371.2e3
    c = CC.case(CC.smooth(37, 40, 12, periodic=True), [0.05, 0.4], periodic=True, radius=R)
    ref = CC.reference(c)
    got = run(ctx, c, 'sphere')
    tol = R * (1e-13 + 1e-13 * ref['dist'] / R)
    assert (np.abs(got['dist'] - ref['dist']) <= tol).all(), float(np.abs(got['dist'] - ref['dist']).max())
    same(run(ctx, c, 'sphere unpruned', prune=False), got, 'sphere unpruned')
    prof = ctx.last_cdist_profile()
    assert prof['pairs_total'] > 0 and prof['pairs_visited'] == prof['pairs_total']


def test_refusals_write_nothing(ctx):
    c = CC.ring_case()
    plain = dict(c, periodic=0)
    for what, case, kw in (('select without periodic', plain, dict(select=1)),
                           ('a sphere with a wrong period', dict(c, radius=1.0), dict(period=6.0))):
        rc, _, untouched = call(ctx, case, **kw)
        assert rc == nat.XC_EBADARG and untouched, what
    cnt, ef, et, pts = c['rec']
    for bad in (2 * c['ny'] * c['nx'], -1):
        ef2 = ef.copy(); ef2[ef.size // 2] = bad
        rc, _, untouched = call(ctx, dict(c, rec=(cnt, ef2, et, pts)))
        assert rc == nat.XC_EBADARG and untouched, 'an id out of range'
    et2 = et.copy(); et2[3] = 2 * c['ny'] * c['nx']
    rc, _, untouched = call(ctx, dict(c, rec=(cnt, ef, et2, pts)))
    assert rc == nat.XC_EBADARG and untouched, 'an e_to out of range'
