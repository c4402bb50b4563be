"""contour_polylines(packed=True), the vectorised vertex builder, against the nested return of the same call (no device): hand-built
records joined by xc_join_segments, every vertex bit for bit, every offset, flag and winding equal.  The last test shows that the
comparison can fail."""
import numpy as np
import pytest

import cpiece_records_ref as RR
from xcontour_amd import _native as nat
from xcontour_amd.core import contour_polylines

NX = 10                                   # the ring of the periodic cases: columns in [0, 10]


def records(ranges, seed=3):
    """ranges: per range a list of (segments [[r1, c1, r2, c2], ...] in walk order, closed) -> (off, e_from, e_to, pts) with the
    ids ascending along every walk (a ring starts at its first segment) and every range stored in a shuffled order"""
    rng = np.random.default_rng(seed)
    off, EF, ET, PT = [0], [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)], [np.zeros((0, 4))]
    for pieces in ranges:
        at, ef, et, pt = 0, [], [], []
        for segs, closed in pieces:
            f, t = RR.chain(np.arange(at, at + len(segs)) * 2 + 1, closed, 1000 + at)
            ef.append(f); et.append(t); pt.append(np.array(segs, dtype=np.float64).reshape(-1, 4)); at += len(segs)
        if at:
            o = rng.permutation(at)
            EF.append(np.concatenate(ef)[o]); ET.append(np.concatenate(et)[o]); PT.append(np.concatenate(pt)[o])
        off.append(off[-1] + at)
    return np.array(off, dtype=np.int64), np.concatenate(EF), np.concatenate(ET), np.concatenate(PT)


def both(ranges, **kw):
    off, ef, et, pts = records(ranges)
    walk, poff, closed, rpo = nat.join_segments(off, ef, et)
    assert walk.size < 2 or not np.array_equal(walk, np.arange(walk.size))          # the gather through `walk` is exercised
    return contour_polylines(walk, poff, closed, rpo, pts, **kw), contour_polylines(walk, poff, closed, rpo, pts, packed=True, **kw)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def compare(nested, packed):
    polys, cl, wd = nested
    verts, voff, pcl, pwd, roff = packed
    assert verts.dtype == np.float64 and verts.ndim == 2 and verts.shape[1] == 2
    assert voff.dtype == np.int64 and roff.dtype == np.int64 and pcl.dtype == np.bool_ and pwd.dtype == np.int64
    assert roff.size == len(polys) + 1 and roff[0] == 0 and voff[0] == 0
    assert np.array_equal(np.diff(roff), [len(p) for p in polys])
    npoly = int(roff[-1])
    assert voff.size == npoly + 1 and pcl.size == npoly and pwd.size == npoly and int(voff[-1]) == verts.shape[0]
    for r, ps in enumerate(polys):
        for k, v in enumerate(ps):
            p = int(roff[r]) + k
            got = verts[voff[p]:voff[p + 1]]
            assert got.shape == v.shape and np.array_equal(bits(got), bits(v)), 'range %d polyline %d' % (r, k)
            assert bool(pcl[p]) == cl[r][k] and int(pwd[p]) == wd[r][k], 'range %d polyline %d' % (r, k)


OPEN3 = ([[0.0, 0.5, 0.5, 1.0], [0.5, 1.0, 1.0, 1.5], [1.0, 1.5, 2.0, 1.5]], False)
RING4 = ([[3.0, 3.5, 3.5, 4.0], [3.5, 4.0, 4.0, 3.5], [4.0, 3.5, 3.5, 3.0], [3.5, 3.0, 3.0, 3.5]], True)
REPEAT = ([[5.0, 0.5, 5.5, 1.0], [5.5, 1.0, 5.5, 1.0], [5.5, 1.0, 6.0, 1.5], [6.0, 1.5, 6.0, 1.5]], False)   # two merged vertices
POINT_OPEN = ([[7.0, 7.0, 7.0, 7.0]], False)                                 # one coincident-end segment: one vertex, dropped
POINT_RING = ([[8.0, 2.0, 8.0, 2.0], [8.0, 2.0, 8.0, 2.0]], True)            # a ring of coincident-end segments: dropped
ONE = ([[2.0, 6.0, 2.5, 6.5]], False)

PLAIN = {
    'open chains, rings and dropped polylines': [[OPEN3, POINT_OPEN, RING4, REPEAT, POINT_RING, ONE]],
    'a dropped polyline first and last': [[POINT_RING, OPEN3, POINT_OPEN]],
    'only dropped polylines': [[POINT_OPEN, POINT_RING]],
    'an empty range': [[]],
    'two ranges, the first empty': [[], [RING4, POINT_OPEN, OPEN3]],
    'ranges with an empty one between': [[OPEN3], [], [POINT_RING], [REPEAT, RING4], []],
}


@pytest.mark.parametrize('coords', [False, True], ids=['index space', 'coordinates'])
@pytest.mark.parametrize('name', list(PLAIN))
def test_packed_equals_nested_on_a_plain_plane(name, coords):
    kw = dict(ycoord=np.linspace(-30.0, 31.0, 12) ** 3 / 900.0, xcoord=np.arange(9.0) * 1.25 + 0.1) if coords else {}
    nested, packed = both(PLAIN[name], **kw)
    compare(nested, packed)
    kept = sum(len(p) for p in nested[0])
    assert kept == {'open chains, rings and dropped polylines': 4, 'a dropped polyline first and last': 1, 'only dropped polylines': 0,
                    'an empty range': 0, 'two ranges, the first empty': 2, 'ranges with an empty one between': 3}[name]


def seam_rings():
    """rings of winding +2, +1, 0 (laps +1 then -1), -1, -2 and an open chain across the seam, columns in [0, NX]"""
    n = float(NX)
    w2 = ([[0.5, 9.0, 0.5, n], [0.5, 0.0, 0.5, 5.0], [0.5, 5.0, 0.5, n], [0.5, 0.0, 0.5, 9.0]], True)
    w1 = ([[1.5, 9.5, 1.25, n], [1.25, 0.0, 1.5, 9.5]], True)
    w0 = ([[2.0, 9.0, 2.0, n], [2.0, 0.0, 2.5, 0.5], [2.5, 0.5, 3.0, 0.0], [3.0, n, 2.0, 9.0]], True)
    m1 = ([[3.5, 0.5, 3.5, 0.0], [3.5, n, 3.5, 0.5]], True)
    m2 = ([[4.5, 1.0, 4.5, 0.0], [4.5, n, 4.5, 5.0], [4.5, 5.0, 4.5, 0.0], [4.5, n, 4.5, 1.0]], True)
    op = ([[5.0, 8.0, 5.5, n], [5.5, 0.0, 5.5, 0.0], [5.5, 0.0, 6.0, 2.0]], False)
    return [w2, w1, w0, m1, m2, op]


@pytest.mark.parametrize('coords', [False, True], ids=['index space', 'coordinates'])
def test_packed_equals_nested_on_a_periodic_plane_with_laps_and_windings(coords):
    kw = dict(nx=NX)
    if coords:
        kw.update(ycoord=np.arange(8.0) * 2.5 - 9.0, xcoord=np.arange(NX) * 36.0 + 0.25, period=360.0)
    ranges = [[], seam_rings(), [POINT_RING] + seam_rings()[::-1]]
    nested, packed = both(ranges, **kw)
    compare(nested, packed)
    assert sorted(nested[2][1]) == [-2, -1, 0, 0, 1, 2] and sorted(packed[3][:6].tolist()) == [-2, -1, 0, 0, 1, 2]
    # the laps are in the vertices: the +2 ring ends two rings on, the -2 ring two rings back
    step = 360.0 if coords else float(NX)
    for ps, ws in zip(nested[0][1:], nested[2][1:]):
        for v, w in zip(ps, ws):
            if w:
                assert v[-1, 1] - v[0, 1] == w * step and v[-1, 0] == v[0, 0]


def unmerged(walk, poff, closed, rpo, pts):
    """a packed builder that forgets to merge consecutive equal vertices (index space, plain plane)"""
    P = np.asarray(pts)[walk]
    vs = [np.concatenate([P[a:a + 1, :2], P[a:b, 2:]]) for a, b in zip(poff[:-1], poff[1:])]
    stays = np.array([len(np.unique(v, axis=0)) >= 2 for v in vs], dtype=bool)
    vs = [v for v, s in zip(vs, stays) if s]
    voff = np.concatenate([[0], np.cumsum([len(v) for v in vs])]).astype(np.int64)
    roff = np.concatenate([[0], np.cumsum(stays)]).astype(np.int64)[rpo]
    return np.concatenate(vs), voff, np.asarray(closed, dtype=bool)[stays], np.zeros(len(vs), dtype=np.int64), roff


def test_a_builder_that_does_not_merge_the_repeated_vertex_is_caught():
    off, ef, et, pts = records([[OPEN3, REPEAT, RING4]])
    walk, poff, closed, rpo = nat.join_segments(off, ef, et)
    nested = contour_polylines(walk, poff, closed, rpo, pts)
    compare(nested, contour_polylines(walk, poff, closed, rpo, pts, packed=True))
    broken = unmerged(walk, poff, closed, rpo, pts)
    assert broken[0].shape[0] == sum(len(v) for v in nested[0][0]) + 2          # REPEAT's two repeated vertices are still there
    with pytest.raises(AssertionError):
        compare(nested, broken)
    # and on records without a repeated vertex the same builder passes: it is the merge that the comparison caught
    off, ef, et, pts = records([[OPEN3, RING4]])
    walk, poff, closed, rpo = nat.join_segments(off, ef, et)
    compare(contour_polylines(walk, poff, closed, rpo, pts), unmerged(walk, poff, closed, rpo, pts))
