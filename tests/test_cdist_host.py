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


GPU_INPUTS = [('diamond', CC.diamond_case, 0), ('ring all', CC.ring_case, 0), ('ring main', CC.ring_case, 2),
              ('37x45', lambda: CC.plane_cases()['37x45'], 0), ('17x33', lambda: CC.plane_cases()['17x33'], 0)]


@pytest.mark.parametrize('wrong', DR.WRONG)
def test_every_wrong_rule_shows_on_the_inputs_of_the_gpu_tests(wrong):
    """each wrong rule changes dist or edge on at least one of the cases the GPU tests compare bit for bit"""
    told = []
    for name, make, select in GPU_INPUTS:
        c = make()
        if wrong == 'no shift' and not c['periodic']:
            continue
        ref, bad = CC.reference(c, select), CC.reference(c, select, wrong=wrong)
        if not DR.same_bits(ref['dist'], bad['dist']) or not np.array_equal(ref['edge'], bad['edge']):
            told.append(name)
    assert told, 'no case tells the rule %r' % wrong


def test_the_sphere_case_tells_a_wrong_rule_beyond_its_tolerance():
    c = CC.case(CC.smooth(20, 24, 4, periodic=True), [0.1], periodic=True, radius=6371.2e3)
    ref = CC.reference(c)
    for wrong in ('no clamp', 'line'):
        bad = CC.reference(c, wrong=wrong)
        assert (np.abs(bad['dist'] - ref['dist']) > c['radius'] * 1e-6).any(), wrong


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
