"""The restatement of K13 (contour_pieces_ref: the pieces of a contour and their statistics) against closed forms, against K10's
restatement and against the host join; and xcontour_amd.contour_area.  No GPU."""
import math

import numpy as np

import clength_ref as CR
import clength_periodic_ref as CPR
import contour_join_ref as JR
import contour_join_periodic_ref as JP
import contour_pieces_ref as PR
import xcontour_amd as xa


def test_contour_area_is_the_shoelace_formula():
    sq = np.array([[1.0, 1.0], [1.0, 4.0], [3.0, 4.0], [3.0, 1.0]])
    assert xa.contour_area(sq) == 6.0
    assert xa.contour_area(sq[::-1]) == 6.0                                      # reversed ring: the same area
    assert xa.contour_area(np.concatenate([sq, sq[:1]])) == 6.0                  # the closing vertex may be repeated
    tri = np.array([[0.0, 0.0], [0.0, 5.0], [2.0, 0.0]])
    assert xa.contour_area(tri) == 5.0 and xa.contour_area(tri[::-1]) == 5.0
    rng = np.random.default_rng(3)
    ang = np.sort(rng.uniform(0.0, 2.0 * np.pi, 17))
    p = np.stack([3.0 + 2.0 * np.sin(ang), 1.0 + 2.0 * np.cos(ang)], axis=1)     # [j, i]
    j, i = p[:, 0], p[:, 1]
    want = 0.5 * abs(math.fsum(i * np.roll(j, -1) - np.roll(i, -1) * j))
    assert abs(xa.contour_area(p) - want) <= 1e-14 * want
    assert xa.contour_area(np.zeros((0, 2))) == 0.0


def test_a_row_field_on_a_periodic_ring_and_on_the_plain_plane():
    ny, nx = 7, 24
    y, x = np.arange(ny) * 2.0 + 1.0, np.arange(nx) * 1.5
    period = nx * 1.5
    q = np.repeat(np.arange(ny, dtype=np.float64)[:, None], nx, axis=1)
    (p,) = PR.pieces(q, [3.25], y, x, period=period)
    assert p.size == 1 and bool(p['closed'][0]) and int(p['nseg'][0]) == nx and abs(int(p['winding'][0])) == 1
    y0 = 1.0 + 2.0 * 3.25
    assert abs(p['length'][0] - period) <= 1e-12 * period
    assert abs(abs(p['area'][0]) - y0 * period) <= 1e-12 * y0 * period
    assert p['row_min'][0] == 3.25 and p['row_max'][0] == 3.25
    # the same plane with two free edges: one open piece
    (p,) = PR.pieces(q, [3.25], y, x)
    assert p.size == 1 and not p['closed'][0] and int(p['nseg'][0]) == nx - 1 and int(p['winding'][0]) == 0
    assert np.isnan(p['area'][0]) and abs(p['length'][0] - (nx - 1) * 1.5) <= 1e-12 * period


def test_a_cone_is_one_ring_whose_area_is_contour_area_of_its_vertices():
    n = 41
    yy, xx = np.meshgrid(np.arange(n) - 20.0, np.arange(n) - 20.0, indexing='ij')
    cone = -np.hypot(yy, xx)
    y, x = np.arange(n) * 0.5, np.arange(n) * 2.0
    (p,) = PR.pieces(cone, [-12.3], y, x)
    assert p.size == 1 and bool(p['closed'][0]) and int(p['winding'][0]) == 0
    (polys,), _ = JR.polylines(cone, [-12.3], y, x)
    want = xa.contour_area(polys[0])
    assert abs(abs(p['area'][0]) - want) <= 1e-12 * want
    assert abs(want - np.pi * 12.3 ** 2) < 0.02 * want                           # and near the disc's (x 0.5 x 2.0 = 1)


def test_the_sign_of_the_area_tells_which_side_is_inside():
    """Both coordinates ascending: S > 0 for a ring that encloses values ABOVE the level (a bump), S < 0 for one that encloses
    values below it (the bump's negative); a descending coordinate flips both."""
    n = 33
    yy, xx = np.meshgrid(np.arange(n) - 16.0, np.arange(n) - 16.0, indexing='ij')
    bump = np.exp(-(yy ** 2 + xx ** 2) / 60.0)
    y, x = np.arange(n) * 1.0, np.arange(n) * 1.0
    (a,) = PR.pieces(bump, [0.5], y, x)
    (b,) = PR.pieces(-bump, [-0.5], y, x)
    assert a.size == 1 and b.size == 1 and a['closed'][0] and b['closed'][0]
    assert a['area'][0] > 0 and b['area'][0] < 0
    assert abs(a['area'][0] + b['area'][0]) <= 1e-12 * a['area'][0]
    (c,) = PR.pieces(bump, [0.5], y[::-1].copy(), x)
    assert c['area'][0] < 0 and abs(c['area'][0] + a['area'][0]) <= 1e-12 * a['area'][0]


def _noise():
    rng = np.random.default_rng(23)
    q = rng.standard_normal((37, 61))
    q[rng.random(q.shape) < 0.03] = np.nan
    lv = np.concatenate([[-9.0], np.linspace(-2.0, 2.0, 5), [np.nan]])
    return q, lv


def test_sums_match_the_length_restatement_and_counts_match_the_join():
    q, lv = _noise()
    ny, nx = q.shape
    for latlon in (False, True):
        y, x = CR.plane_coords(np.linspace(-60.0, 60.0, ny), np.arange(nx) * 2.5, latlon)
        for period in (None, float(x[1] - x[0]) * nx):
            P = PR.pieces(q, lv, y, x, latlon, period)
            if period is None:
                tot, cnt = CR.contour_lengths(q, lv, y, x, latlon)
                polys, closed = JR.polylines(q, lv)[:2]
                census = JP.census(q, lv, periodic=False)
            else:
                tot, cnt = CPR.contour_lengths(q, lv, y, x, period, latlon)
                polys, closed = JP.polylines(q, lv)[:2]
                census = JP.census(q, lv)
            for k in range(lv.size):
                if np.isnan(tot[k]):
                    assert P[k]['length'].sum() == 0.0
                    continue
                s = math.fsum(P[k]['length'])
                assert abs(s - tot[k]) <= 1e-12 * tot[k], (latlon, period, k)
                # every joined polyline is a piece (this field has none that find_contours would drop)
                assert P[k].size == len(census[k]) == len(polys[k])
                assert P[k]['closed'].tolist() == [bool(c) for c in closed[k]]
                assert sorted((int(n), bool(c), int(w)) for n, c, w in census[k]) == \
                    sorted(zip(P[k]['nseg'].tolist(), P[k]['closed'].tolist(), P[k]['winding'].tolist()))
            assert P[0].size == 0 and P[-1].size == 0
