"""xc_contour_distance_dev (K27) where its block scan, its pruning and its tie rule can fail (cdist_cases; test_cdist_host.py shows on
the CPU what each case holds): planes of more than 256 blocks, which the scan of k_cd_scan takes in more than one chunk; a tie between
two blocks; the sphere from pole to pole on descending coordinates; empty ranges before and between the others; a cap that rules whole
tiles out.  On the plane dist BIT FOR BIT, edge and piece equal, as in test_gpu_cdist_records.py, whose call (pattern-filled outputs,
guard elements) every run here goes through.

Pruning is pinned by COUNT as well as by result.  pairs_total is nodes x selected segments by its definition; an unpruned call visits
all of them; and on the plane pairs_visited is the count of cdist_ref.pruned, which walks the blocks in the same ascending order
under the same bounds -- so a kernel that skips too little shows as well as one that skips too much.  Every call prints its counts."""
import numpy as np
import pytest

import cdist_cases as CC
import cdist_ref as DR
from test_gpu_cdist_records import run, same

pytestmark = pytest.mark.gpu


def counts(ctx):
    p = ctx.last_cdist_profile()
    return p['pairs_visited'], p['pairs_total']


def variants(ctx, c, what, select=0, model=None, strict=False, **kw):
    """the call as it stands, unpruned and with one range per group: the same bits, and the pair counts by their definitions.
    model: the pairs cdist_ref.pruned visits (plane, every segment selected, no cap); strict: pruning must skip something.
    -> (the pruned call's result, its pairs_visited)"""
    total = c['ny'] * c['nx'] * CC.nselected(c, select)
    got = run(ctx, c, what, select, **kw)
    visited, t = counts(ctx)
    print('%s, select %d: pairs_visited / pairs_total = %d / %d = %.4f%s' % (what, select, visited, t, visited / max(t, 1),
                                                                          '' if model is None else ', the model visits %d' % model))
    assert t == total, 'pairs_total is not nodes x selected segments'
    assert visited <= total
    un = run(ctx, c, what + ' unpruned', select, prune=False, **kw)
    assert counts(ctx) == (total, total), 'an unpruned call visits every pair'
    same(un, got, what + ' unpruned')
    one = run(ctx, c, what + ' one range per group', select, cap=1, **kw)
    assert counts(ctx) == (visited, total), 'the pairs depend on the workspace cap'
    same(one, got, what + ' one range per group')
    if strict:
        assert visited < total, 'nothing was pruned'
    if model is not None:
        assert visited == model, 'the kernel and the model walk differently'
    return got, visited


def empty_planes(c, got):
    """every range without segments: +inf, -1, -1 -> how many there are"""
    empty = np.flatnonzero(c['rec'][0].ravel() == 0)
    for r in empty:
        assert np.isposinf(got['dist'][r]).all() and (got['edge'][r] == -1).all() and (got['piece'][r] == -1).all(), r
    return empty.size


def model_planes(name):
    """cdist_ref.pruned on every range as the planes of a call: (dist, edge), and its pairs"""
    per_range, pairs = CC.model(name)
    return np.stack([np.sqrt(d2) for d2, _ in per_range]), np.stack([e for _, e in per_range]), pairs


def test_1x258_blocks_the_whole_plane(ctx):
    """2 x 8225: the scan's second chunk holds blocks 256 and 257; the empty range comes first"""
    name = '2x8225'
    c = CC.wide_case()
    assert name in CC.PRUNED_FOR_SURE
    _, _, pairs = model_planes(name)
    got, _ = variants(ctx, c, name, model=pairs, strict=True)
    same(got, CC.cached_reference(name), name)
    assert empty_planes(c, got) == 1 and c['rec'][0].ravel()[0] == 0


def test_2x130_blocks_the_chunk_boundary_inside_a_block_row(ctx):
    """34 x 4130 on the ring, two ranges in one group: against the brute force on the nodes around blocks 255 and 256 and every
    7th elsewhere, and over the whole plane against the model's walk (test_cdist_host.py: the brute force's bits on those nodes)"""
    name = '34x4130 ring'
    c = CC.wide_ring_case()
    assert name in CC.PRUNED_FOR_SURE
    dist, edge, pairs = model_planes(name)
    got, _ = variants(ctx, c, name, model=pairs, strict=True)
    at = np.ix_(np.arange(2), *CC.wide_ring_nodes())
    same({k: v[at] for k, v in got.items()}, CC.cached_reference(name, 0, 0.0, 'wide_ring_nodes'), name + ' on the subset')
    assert DR.same_bits(got['dist'], dist) and np.array_equal(got['edge'], edge), 'the whole plane against the model'


def test_a_tie_across_two_blocks_goes_to_the_smaller_id(ctx):
    """node (0, 31) is exactly 25 from P0 (block 0) and from P1 (block 1, the smaller id); block 1's lower bound EQUALS the tile's
    bound, 625: a skip rule that is not strict returns P0"""
    base = CC.cross_block_tie_case()
    p0, p1 = [int(v) for v in base['rec'][1]]
    _, pairs = CC.model('cross-block tie')
    for what, c in (('tie', base), ('tie swapped', CC.swapped(base))):
        got, _ = variants(ctx, c, what, model=pairs)
        same(got, CC.reference(c), what)
        assert got['dist'][0, 0, 31] == 25.0 and got['edge'][0, 0, 31] == p1 and got['piece'][0, 0, 31] == p1
        assert got['edge'][0, 20, 16] == p0 and got['dist'][0, 20, 16] == 0.0


@pytest.mark.parametrize('name', ['37x45', '37x45 noise', '37x40 ring noise', 'ring', '37x45 down', '37x40 ring down'])
def test_pair_counts_and_descending_coordinates(ctx, name):
    """the earlier cases by count, and the planes whose ycoord and xcoord both descend (on the ring: a negative period, column nx
    one period BELOW column 0), bit for bit"""
    c = CC.any_case(name)
    dist, edge, pairs = model_planes(name)
    got, _ = variants(ctx, c, name, model=pairs)
    same(got, CC.cached_reference(name), name)
    assert DR.same_bits(got['dist'], dist) and np.array_equal(got['edge'], edge)
    if c['periodic'] and name != '37x40 ring noise':
        main, _ = variants(ctx, c, name + ' main', select=2)
        same(main, CC.cached_reference(name, 2), name + ' main')


def nearest_is_consistent(c, select, r, got, tol):
    """the returned edge is a selected segment, the restatement's distance from every node to it ALONE is the returned dist within
    the bound, and piece is that segment's piece"""
    ef = np.asarray(c['rec'][1], dtype=np.int64)
    idx, first = DR.selected(*c['rec'], c['ny'], c['nx'], c['periodic'], select)[r]
    e = got['edge'][r].ravel()
    k = np.minimum(np.searchsorted(ef[idx], e), idx.size - 1)
    assert np.array_equal(ef[idx][k], e), 'an edge that is not a selected segment'
    assert np.array_equal(got['piece'][r].ravel(), first[k])
    Y1, X1, Y2, X2 = [v[idx][k] for v in DR.end_points(c['rec'][3], c['ny'], c['nx'], c['ycoord'], c['xcoord'], True, c['period'])]
    PY, PX = [v.ravel() for v in np.meshgrid(c['ycoord'], c['xcoord'], indexing='ij')]
    c2 = DR.c2_sphere(DR.unit(PY, PX)[:, None, :], DR.unit(Y1, X1)[:, None, :], DR.unit(Y2, X2)[:, None, :])[:, 0]
    assert (np.abs(DR.finish(c2, c['radius']) - got['dist'][r].ravel()) <= tol.ravel()).all()


@pytest.mark.parametrize('select', [0, 2])
@pytest.mark.parametrize('name', sorted(CC.sphere_cases()))
def test_the_sphere_from_pole_to_pole(ctx, name, select):
    """70 x 100, 3 x 4 blocks: latitudes descending from +90 to -90 degrees, longitudes of either sense (period +-RING).  Within
    R (1e-13 + 1e-13 ref / R), the bound test_gpu_cdist.py derives; the sphere's slack prunes (no model of its bounds: the kernel's
    own count), and pruned and unpruned agree in every bit; a pole row is one point.  (With the segment's normal taken as a x b
    this missed the bound, 8.6e-7 m against 6.4e-7 m, at nodes whose nearest segment cuts a cell's corner, |n| near 1e-5: the
    normal is a x (b - a) since, and the largest difference is 1.3e-8 m.)"""
    c = CC.sphere_cases()[name]
    R = c['radius']
    ref = CC.cached_reference(name, select)
    got, _ = variants(ctx, c, name, select, strict=True)
    tol = R * (1e-13 + 1e-13 * ref['dist'] / R)
    err = np.abs(got['dist'] - ref['dist'])
    worst = np.unravel_index(err.argmax(), err.shape)
    print('%s, select %d: max |dist - ref| = %.3e m at (range, row, col) = %r, ref there %.6e m, bound there %.3e m; %d nodes beyond the bound'
          % (name, select, float(err.max()), tuple(int(v) for v in worst), float(ref['dist'][worst]), float(tol[worst]), int((err > tol).sum())))
    for k in np.argwhere(err > tol)[:12]:
        print('   beyond the bound at %r: |dist - ref| = %.3e m, ref %.6e m, edge %d (ref %d)'
              % (tuple(int(v) for v in k), float(err[tuple(k)]), float(ref['dist'][tuple(k)]), int(got['edge'][tuple(k)]), int(ref['edge'][tuple(k)])))
    assert (err <= tol).all()
    for r in range(2):
        nearest_is_consistent(c, select, r, got, tol[r])
    for row in (0, -1):
        first = got['dist'][:, row, :1]
        assert (np.abs(got['dist'][:, row, :] - first) <= R * (1e-13 + 1e-13 * first / R)).all(), 'the pole row %d' % row


@pytest.mark.parametrize('cap', [None, 1], ids=['one group', 'one range per group'])
@pytest.mark.parametrize('name', ['37x45 empty around', '70x530 ring'])
def test_empty_ranges_before_between_and_after(ctx, name, cap):
    """levels 99, -0.4, 99, 0.1, 99: k_cd_none writes the planes before the first group, between two groups (one range per group)
    and after the last; the others are the reference's bits and no guard is touched (call)"""
    c = CC.geometry_cases()[name]
    assert (c['rec'][0].ravel() > 0).tolist() == [False, True, False, True, False]
    got = run(ctx, c, name, cap=cap)
    visited, total = counts(ctx)
    same(got, CC.cached_reference(name), name)
    assert empty_planes(c, got) == 3
    assert total == c['ny'] * c['nx'] * CC.nselected(c) and visited == CC.model(name)[1]
    if name in CC.PRUNED_FOR_SURE:
        assert visited < total


def test_a_cap_that_rules_whole_tiles_out(ctx):
    """70 x 530 on the ring, max_dist = the 10th percentile of the reference's distances: most tiles lie beyond it altogether.
    With a negate_mask of random bits: a capped node stays +inf, never -inf"""
    name = '70x530 ring'
    c = CC.geometry_cases()[name]
    ref = CC.cached_reference(name)
    cap = float(np.percentile(ref['dist'][np.isfinite(ref['dist'])], 10))
    mask = CC.random_mask(c, 5)
    refc = CC.cached_reference(name, 0, cap, None, 5)
    gone = np.isposinf(refc['dist'][1])
    assert any(gone[r:r + DR.TILE, k:k + DR.TILE].all() for r in range(0, 70, DR.TILE) for k in range(0, 530, DR.TILE)), 'no whole tile is capped'
    assert (refc['dist'] < 0).any() and not np.isneginf(refc['dist']).any() and (gone & (mask[1] != 0)).any()
    plain, visited = variants(ctx, c, name, strict=True)
    for prune in (True, False):
        got = run(ctx, c, name + ' capped', max_dist=cap, mask=mask, prune=prune)
        v, t = counts(ctx)
        print('%s, max_dist %.4g, prune %r: pairs_visited / pairs_total = %d / %d' % (name, cap, prune, v, t))
        same(got, refc, '%s capped, prune %r' % (name, prune))
        assert not np.isneginf(got['dist']).any()
        assert t == c['ny'] * c['nx'] * CC.nselected(c)
        assert v <= visited if prune else v == t
