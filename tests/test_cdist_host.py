"""cdist_ref, the numpy restatement of K27 (distance to a contour), on values worked out by hand, and against deliberately wrong
rules on the very inputs the GPU tests run (cdist_cases): none of those can pass vacuously.  No GPU here."""
import numpy as np
import pytest

import cdist_cases as CC
import cdist_ref as DR


def one_segment(a, b, nodes, periodic=False, period=0.0, radius=0.0, **kw):
    """the distance from each node (y, x) to the one segment a -> b, on coordinates that ARE the values given"""
    ys = sorted({p[0] for p in nodes} | {a[0], b[0]})
    xs = sorted({p[1] for p in nodes} | {a[1], b[1]})
    ny, nx = len(ys), len(xs)
    at = lambda p: (float(ys.index(p[0])), float(xs.index(p[1])))
    rec = (np.array([1], dtype=np.uint64), np.array([0]), np.array([2]), np.array([at(a) + at(b)]))
    out = DR.distance(*rec, ny, nx, periodic, 0, np.array(ys), np.array(xs), period, radius, **kw)
    return np.array([out['dist'][0, ys.index(p[0]), xs.index(p[1])] for p in nodes])


def test_three_four_five_and_the_ends_of_a_segment():
    d = one_segment((0.0, 0.0), (0.0, 8.0), [(3.0, 4.0), (0.0, 5.0), (3.0, 12.0), (-4.0, -3.0)])
    assert d.tolist() == [3.0, 0.0, 5.0, 5.0]              # over the segment; on it; beyond b (3-4-5); beyond a (4-3-5)
    d = one_segment((1.0, 1.0), (1.0, 1.0), [(4.0, 5.0)])  # coincident ends: the point
    assert d.tolist() == [5.0]


def test_the_smaller_id_wins_a_tie_and_the_diamond_is_exact():
    c = CC.diamond_case()
    ref = CC.reference(c)
    assert ref['dist'][0, 8, 8] == np.sqrt(8.0) and ref['edge'][0, 8, 8] == c['rec'][1][:4].min()
    assert ref['piece'][0, 8, 8] == c['rec'][1][:4].min()
    assert ref['dist'][0, 14, 22] == 0.0 and ref['dist'][0, 14, 30] == 6.0 and ref['dist'][0, 16, 24] == 2.0
    assert ref['piece'][0, 14, 30] == c['rec'][1][4]
    wrong = CC.reference(c, wrong='tie larger')
    assert wrong['edge'][0, 8, 8] == c['rec'][1][:4].max()


def test_the_image_across_the_seam_is_nearer():
    d = one_segment((0.0, 1.0), (0.0, 2.0), [(0.0, 9.0)], periodic=True, period=10.0)
    assert d.tolist() == [2.0]                             # 9 -> -1 by one period
    assert one_segment((0.0, 1.0), (0.0, 2.0), [(0.0, 9.0)], periodic=True, period=10.0, wrong='no shift').tolist() == [7.0]


def test_sphere_pole_and_antipode():
    lat = np.deg2rad(60.0)
    # the pole against a segment between two points of one parallel: the segment is the great-circle arc, whose highest point, over
    # the middle longitude, lies at atan(tan(lat) / cos(dlon / 2)) -- the colatitude of the parallel to second order in dlon
    d = one_segment((lat, 0.1), (lat, 0.2), [(np.pi / 2, 0.15)], radius=2.0)
    top = np.arctan(np.tan(lat) / np.cos(0.05))
    assert abs(d[0] - 2.0 * (np.pi / 2 - top)) < 1e-14 and abs(d[0] - 2.0 * (np.pi / 2 - lat)) < 2.0 * 0.1 ** 2
    d = one_segment((0.0, 0.0), (0.0, 0.0), [(0.0, np.pi)], radius=1.0)
    assert abs(d[0] - np.pi) < 1e-7 and np.isfinite(d[0])   # antipodal to the (point) segment: asin's argument is clamped at 1
    d = one_segment((0.0, 0.0), (0.0, 1.0), [(0.5, 0.5), (0.0, 1.5)], radius=1.0)
    assert abs(d[0] - 0.5) < 1e-14 and abs(d[1] - 0.5) < 1e-14          # over the arc of the equator; beyond its end


def test_cap_and_sign():
    c = CC.diamond_case()
    ref = CC.reference(c)
    cap = CC.reference(c, max_dist=3.0)
    far = ref['dist'] > 3.0
    assert far.any() and (~far).any()
    assert np.isinf(cap['dist'][far]).all() and (cap['edge'][far] == -1).all() and (cap['piece'][far] == -1).all()
    assert DR.same_bits(cap['dist'][~far], ref['dist'][~far])
    mask = np.zeros((1, c['ny'], c['nx']), dtype=np.uint8); mask[0, :9] = 1
    neg = CC.reference(c, negate_mask=mask)
    assert DR.same_bits(neg['dist'][0, :9], -ref['dist'][0, :9]) and DR.same_bits(neg['dist'][0, 9:], ref['dist'][0, 9:])


def test_a_negative_period_puts_column_nx_below_column_zero():
    """descending coordinates on a ring: xcoord = 9, 7, 5, 3, 1 and period -10, so column 5 lies at 9 - 10 = -1; ycoord = 3, 0.  The
    one segment runs on row 0 (y = 3) from column 4.5 to column 5, across the seam: x from 0 to -1.  Node (row 1, column 0) = (0, 9)
    is nearest through its image 9 - 10 = -1, right under the segment's end: 3 away; without images sqrt(81 + 9).  Node (row 1,
    column 4) = (0, 1) has the foot at the segment's start: sqrt(9 + 1)."""
    y, x = np.array([3.0, 0.0]), np.array([9.0, 7.0, 5.0, 3.0, 1.0])
    rec = (np.array([1], dtype=np.uint64), np.array([8]), np.array([9]), np.array([(0.0, 4.5, 0.0, 5.0)]))
    assert [float(v[0]) for v in DR.end_points(rec[3], 2, 5, y, x, True, -10.0)] == [3.0, 0.0, 3.0, -1.0]
    out = DR.distance(*rec, 2, 5, True, 0, y, x, -10.0)
    assert out['dist'][0, 1, 0] == 3.0 and out['dist'][0, 1, 4] == np.sqrt(10.0) and out['dist'][0, 0, 4] == 1.0
    assert DR.distance(*rec, 2, 5, True, 0, y, x, -10.0, wrong='no shift')['dist'][0, 1, 0] == np.sqrt(90.0)
    got, _, edge, pos = DR.pruned(rec[1], rec[3], 2, 5, y, x, True, -10.0, nearest=True)
    assert DR.same_bits(got, out['best'][0]) and (edge == 8).all() and (pos == 0).all()


def test_descending_cases_are_the_ascending_ones_mirrored():
    """the descending record cases hold the same coordinate values from the top down, and a negative period on the ring"""
    for name, periodic in (('37x45 down', False), ('37x40 ring down', True)):
        c = CC.geometry_cases()[name]
        assert (np.diff(c['ycoord']) < 0).all() and (np.diff(c['xcoord']) < 0).all()
        assert (c['period'] < 0.0) if periodic else (c['period'] == 0.0)
        assert c['xcoord'][-1] > c['xcoord'][0] + c['period'] if periodic else True     # column nx goes on downwards
    y, x, p = CC.coords(37, 40, 103, True)
    yd, xd, pd = CC.coords(37, 40, 103, True, descending=True)
    assert np.array_equal(yd, y[::-1]) and np.array_equal(xd, x[::-1]) and pd == -p and p > 0.0 and (np.diff(y) > 0).all()


def test_the_cross_block_tie_is_exact_and_only_a_strict_skip_finds_it():
    c = CC.cross_block_tie_case()
    cnt, ef, et, pts = c['rec']
    p0, p1 = int(ef[0]), int(ef[1])
    assert p1 < p0 and CC.blocks_of(c).tolist() == [0, 1]
    for cc in (c, CC.swapped(c)):
        ref = CC.reference(cc)
        assert ref['dist'][0, 0, 31] == 25.0 and ref['edge'][0, 0, 31] == p1 and ref['piece'][0, 0, 31] == p1
        assert ref['dist'][0, 20, 16] == 0.0 and ref['edge'][0, 20, 16] == p0 and ref['dist'][0, 0, 56] == 0.0
        assert CC.reference(cc, wrong='tie larger')['edge'][0, 0, 31] == p0
        args = (cc['rec'][1], cc['rec'][3], c['ny'], c['nx'], c['ycoord'], c['xcoord'])
        d2, pairs, edge, pos = DR.pruned(*args, nearest=True)
        assert DR.same_bits(d2, ref['best'][0]) and np.array_equal(edge, ref['edge'][0])
        assert np.array_equal(cc['rec'][1][pos], edge)
        assert d2[0, 31] == 625.0 and edge[0, 31] == p1
        d2s, fewer, edges, _ = DR.pruned(*args, bound='gap skip ties', nearest=True)
        assert d2s[0, 31] == 625.0 and edges[0, 31] == p0 and fewer < pairs        # the same distance, the wrong segment


#: (name, the case, select, the nodes compared: None or the name of a function of cdist_cases)
GPU_INPUTS = [('diamond', CC.diamond_case, 0, None), ('ring all', CC.ring_case, 0, None), ('ring main', CC.ring_case, 2, None),
              ('37x45', lambda: CC.plane_cases()['37x45'], 0, None), ('17x33', lambda: CC.plane_cases()['17x33'], 0, None),
              ('cross-block tie', CC.cross_block_tie_case, 0, None), ('2x8225', CC.wide_case, 0, None),
              ('34x4130 ring', CC.wide_ring_case, 0, 'wide_ring_nodes'), ('70x530 ring', lambda: CC.geometry_cases()['70x530 ring'], 0, 'sparse_530_nodes'),
              ('37x45 empty around', lambda: CC.geometry_cases()['37x45 empty around'], 0, None),
              ('37x45 down', lambda: CC.geometry_cases()['37x45 down'], 0, None),
              ('37x40 ring down', lambda: CC.geometry_cases()['37x40 ring down'], 0, None)]
#: the cases whose reference is dear: one wrong rule each, the one they are there to tell
ONLY = {'34x4130 ring': 'no shift', '70x530 ring': 'no shift', '2x8225': 'no clamp'}


@pytest.mark.parametrize('wrong', DR.WRONG)
def test_every_wrong_rule_shows_on_the_inputs_of_the_gpu_tests(wrong):
    """each wrong rule changes dist or edge on at least one of the cases the GPU tests compare bit for bit; every ring tells a
    missing image shift, descending coordinates and a negative period included"""
    told = []
    for name, make, select, nodes in GPU_INPUTS:
        c = make()
        if (wrong == 'no shift' and not c['periodic']) or ONLY.get(name, wrong) != wrong:
            continue
        kw = {} if nodes is None else dict(nodes=getattr(CC, nodes)())
        ref = CC.cached_reference(name, select, 0.0, nodes) if name in ONLY else CC.reference(c, select, **kw)
        bad = CC.reference(c, select, wrong=wrong, **kw)
        if not DR.same_bits(ref['dist'], bad['dist']) or not np.array_equal(ref['edge'], bad['edge']):
            told.append(name)
        else:
            assert wrong != 'no shift' and name not in ONLY, '%s does not tell the rule %r' % (name, wrong)
    assert told, 'no case tells the rule %r' % wrong


def test_every_case_of_the_geometry_tests_is_listed_above():
    listed = {name for name, _, _, _ in GPU_INPUTS}
    assert set(CC.geometry_cases()) <= listed


def test_the_sphere_case_tells_a_wrong_rule_beyond_its_tolerance():
    c = CC.case(CC.smooth(20, 24, 4, periodic=True), [0.1], periodic=True, radius=6371.2e3)
    ref = CC.reference(c)
    for wrong in ('no clamp', 'line'):
        bad = CC.reference(c, wrong=wrong)
        assert (np.abs(bad['dist'] - ref['dist']) > c['radius'] * 1e-6).any(), wrong


def test_the_pole_to_pole_sphere_cases_have_rings_and_tell_a_wrong_rule():
    """descending latitudes with both poles exactly, either sense of longitude: each level has a circumpolar ring (select 2 finds a
    main one), every node of a pole row is the same point within rounding, and both sphere rules show beyond the tolerance"""
    for name, c in sorted(CC.sphere_cases().items()):
        assert c['ycoord'][0] == np.pi / 2 and c['ycoord'][-1] == -np.pi / 2 and (np.diff(c['ycoord']) < 0).all()
        assert c['period'] == (-DR.RING if 'lon down' in name else DR.RING) and np.sign(np.diff(c['xcoord'])).tolist() == [np.sign(c['period'])] * 99
        ref, main = CC.cached_reference(name), CC.cached_reference(name, 2)
        assert np.isfinite(ref['dist']).all() and np.isfinite(main['dist']).all()
        assert not np.array_equal(ref['edge'], main['edge'])                    # the levels have more than their main rings
        for row in (0, -1):
            first = ref['dist'][:, row, :1]
            assert (np.abs(ref['dist'][:, row, :] - first) <= c['radius'] * (1e-13 + 1e-13 * first / c['radius'])).all()
        bad = CC.reference(c, wrong='no clamp')
        assert (np.abs(bad['dist'] - ref['dist']) > c['radius'] * 1e-6).any()


def test_the_wide_planes_fill_blocks_on_both_sides_of_the_scan_chunk():
    """2 x 8225 (1 x 258 blocks) and 34 x 4130 (2 x 130): in every non-empty range blocks below index 256 and at or above it hold
    segments, with an empty block between two of them -- the second chunk of k_cd_scan, its carry and the compacted list all run"""
    for c in (CC.wide_case(), CC.wide_ring_case()):
        assert CC.nblocks(c) > 256
        for r in np.flatnonzero(c['rec'][0].ravel()):
            assert CC.straddles_the_scan_chunk(c, r)
    c = CC.wide_case()
    assert c['rec'][0].ravel().tolist() == [0, 1653, 1776] and np.unique(CC.blocks_of(c, 1)).size == 163


@pytest.mark.parametrize('name', CC.PRUNED_FOR_SURE)
def test_the_model_prunes_on_the_cases_whose_gpu_test_says_the_kernel_does(name):
    """cdist_ref.pruned on every range of the case: the brute-force d2 and winner, bit for bit, over strictly fewer pairs than
    nodes x segments -- the GPU test may ask the kernel for `pairs_visited < pairs_total` there"""
    c = CC.any_case(name)
    nodes = {'34x4130 ring': 'wide_ring_nodes', '70x530 ring': 'sparse_530_nodes'}.get(name)  # (the GPU tests take the model's whole plane)
    ref = CC.cached_reference(name, 0, 0.0, nodes)
    at = np.ix_(*getattr(CC, nodes)()) if nodes else np.ix_(np.arange(c['ny']), np.arange(c['nx']))
    per_range, pairs = CC.model(name)
    for r, (d2, edge) in enumerate(per_range):
        assert DR.same_bits(d2[at], ref['best'][r]) and np.array_equal(edge[at], ref['edge'][r]), r
    assert 0 < pairs < c['ny'] * c['nx'] * CC.nselected(c)


@pytest.mark.parametrize('name', ['37x45', '37x40 ring noise'])
def test_box_bounds_prune_nothing_that_wins_and_centre_distances_do(name):
    """the kernel's tile / block walk restated: with the box-to-box bounds the result is the brute-force one, bit for bit, over
    fewer pairs; with the distance of the box centres for a lower bound it is not"""
    c = CC.plane_cases()[name]
    cnt, ef, et, pts = c['rec']
    n0 = int(cnt.ravel()[0])
    one = (cnt.ravel()[:1], ef[:n0], et[:n0], pts[:n0])
    ref = DR.distance(*one, c['ny'], c['nx'], c['periodic'], 0, c['ycoord'], c['xcoord'], c['period'])['best'][0]
    got, pairs = DR.pruned(ef[:n0], pts[:n0], c['ny'], c['nx'], c['ycoord'], c['xcoord'], c['periodic'], c['period'])
    assert DR.same_bits(got, ref)
    assert pairs <= c['ny'] * c['nx'] * n0
    bad, fewer = DR.pruned(ef[:n0], pts[:n0], c['ny'], c['nx'], c['ycoord'], c['xcoord'], c['periodic'], c['period'], bound='centre')
    assert not DR.same_bits(bad, ref) and fewer < pairs


# ------------------------------------------------------------------ the host layer over a stand-in library
import cdist_standin as ST                                                    # noqa: E402
from xcontour_amd import _native as nat                                       # noqa: E402

S, NY, NX = 2, 6, 8
LV = np.array([-0.5, 0.0, 0.5])
Y, X = np.arange(NY, dtype=np.float64), np.arange(NX, dtype=np.float64)


@pytest.fixture
def sctx():
    c = nat.Context.__new__(nat.Context)
    c.lib, c.handle, c.device = ST.Lib(), None, 0
    c._buffers, c._resident, c._staged, c._ev_pool = [], {}, [], []
    c.max_batch_bytes = 8 << 30
    return c


def _segments(lib, a):
    """a scripted K12: two segments in every range"""
    if a[9]:
        return 0
    lib.poke(a[10], np.full(a[3] * a[7], 2, dtype=np.uint64))
    return 1


@pytest.mark.parametrize('kw,text', [
    (dict(select='main'), 'needs periodic=True'),
    (dict(radius=1.0, period=9.0), 'on the sphere the period is'),
    (dict(radius=-1.0), 'radius must be finite and >= 0'),
    (dict(max_distance=float('nan')), 'max_distance is NaN'),
    (dict(period=3.0), 'period must be finite'),
    (dict(ycoord=np.arange(NY + 1.0)), 'coordinates of length'),
    (dict(xcoord=np.where(X == 3, np.inf, X)), 'coordinates must be finite'),
])
def test_refusals_of_the_binding_reach_no_kernel(sctx, kw, text):
    q = np.zeros((S, NY, NX))
    args = dict(ycoord=Y, xcoord=X)
    args.update(kw)
    with pytest.raises(nat.XContourHipError, match=text):
        sctx.contour_distance(q, LV, args.pop('ycoord'), args.pop('xcoord'), **args)
    assert sctx.lib.calls == []


def test_signed_hands_the_mask_of_k17_to_k27_on_the_device(sctx):
    sctx.lib.on.update({k: _segments for k in ST.SL._K12})
    q = np.zeros((S, NY, NX))
    d, e, p = sctx.contour_distance(q, LV, Y, X, period=NX + 1.0, select='main', max_distance=4.0, signed=True, flip=True, return_nearest=True)
    assert d.shape == e.shape == p.shape == (S, 3, NY, NX) and d.dtype == np.float64 and e.dtype == p.dtype == np.int64
    names = [c[0] for c in sctx.lib.calls]
    assert names == ['xc_contour_segments_periodic_dev'] * 2 + ['xc_contour_interior_dev', ST.K27]
    k17, k27 = sctx.lib.args[2][1], sctx.lib.args[3][1]
    assert k17[1] == k27[1] == S * 3 and k17[8:12] == (1, 2, 1, 3) and k17[12:16] == (None, 0, None, 0)
    assert k27[8:10] == (1, 2) and k27[12:15] == (NX + 1.0, 0.0, 4.0)
    assert k27[15] == k17[19] and k27[15] is not None                          # negate_mask IS K17's mask
    assert sctx.lib.where(k27[15])[1] == S * 3 * NY * NX
    assert [sctx.lib.where(v)[1] for v in k27[16:19]] == [S * 3 * NY * NX * 8] * 3


def test_contours_go_in_groups_under_the_batch_cap(sctx):
    sctx.lib.on.update({k: _segments for k in ST.SL._K12})
    sctx.max_batch_bytes = NY * NX * 8 * 2                                     # two output planes per batch: one slab of two contours
    d = sctx.contour_distance(np.zeros((S, NY, NX)), LV, Y, X)
    assert d.shape == (S, 3, NY, NX)
    k27 = [c for c in sctx.lib.calls if c[0] == ST.K27]
    assert sorted(n for _, n in k27) == [1, 1, 2, 2] and all(a[1][15] is None and a[1][17] is None for a in sctx.lib.args if a[0] == ST.K27)
