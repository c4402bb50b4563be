"""Contour2D.cal_contour_piece_props (K21) on the GPU against the library's own map: the fields of cal_contour_piece_tree byte for byte,
every `<name>_net` math.fsum over the nodes cal_contour_piece_labels gives the ring, every `<name>` the same over the ring and its
descendants, bit for bit (the moments likewise); the centroid the documented formula on the returned moments, bit for bit; the extrema
and their coordinates np.nanmin / np.nanmax over the labels, the gross ones over the subtree."""
import math

import numpy as np
import pytest

import cptree_cases as CS
import xcontour_amd as xa
from test_gpu_cpinside_records import scaled
from test_gpu_cptree import contour2d

pytestmark = pytest.mark.gpu


def fsum(v):
    return math.fsum(float(a) for a in v if a == a)


def same(a, b):
    return (a == b and np.signbit(a) == np.signbit(b)) or (a != a and b != b)


def subtree(t, p):
    """the rows of t whose chain of parents meets p (p itself included)"""
    under, q = np.zeros(t.size, dtype=bool), np.arange(t.size)
    for _ in range(int(t['depth'].max()) + 1):
        under |= q == p
        q = np.where(q >= 0, t['parent'][np.maximum(q, 0)], -1)
    return np.flatnonzero(under)


def against_the_map(t, tree, lab, dA, planes, xv, y, x):
    """one level: t the props table, tree cal_contour_piece_tree's, lab the label map; planes name -> (ny, nx) float64; xv or None"""
    assert all(t[k].tobytes() == tree[k].tobytes() for k in tree.dtype.names) and t.dtype.names[:len(tree.dtype.names)] == tree.dtype.names
    nx = x.size
    for p in range(t.size):
        if not t['closed'][p]:
            assert all(np.isnan(t[k][p]) for k in t.dtype.names[len(tree.dtype.names):]), p
            continue
        net, gross = lab == p, np.isin(lab, subtree(t, p))
        for name, g in planes.items():
            assert same(t[name + '_net'][p], fsum((dA * g)[net])), (name, p)
            assert same(t[name][p], fsum((dA * g)[gross])), (name, p)
        if xv is None:
            continue
        for sel, sfx in ((net, '_net'), (gross, '')):
            v = np.where(sel, xv, np.nan)
            if np.isnan(v).all():
                assert all(np.isnan(t[k + sfx + e][p]) for k in ('vmin', 'vmax') for e in ('', '_y', '_x')), p
                continue
            for k, fn, arg in (('vmin', np.nanmin, np.nanargmin), ('vmax', np.nanmax, np.nanargmax)):
                assert t[k + sfx][p] == fn(v), (k, p)
                at = int(np.flatnonzero(v.ravel() == fn(v))[0])              # of equal values the smallest flat node
                assert t[k + sfx + '_y'][p] == y[at // nx] and t[k + sfx + '_x'][p] == x[at % nx], (k, sfx, p)


def test_the_barotropic_field_at_five_levels_both_sides(baro):
    q, lat, lon = (np.asarray(a, dtype=np.float64) for a in baro)
    q = q[0] if q.ndim == 3 else q
    ny, nx = q.shape
    rng = np.random.default_rng(7)
    # weights in [1, 2): the smallest moment term, cos(lat) cos(lon) ~ 2^-61, then lies wholly inside its 160-bit window like every other term
    dA, g1, g2 = rng.uniform(1.0, 2.0, (ny, nx)), scaled(rng, (ny, nx)), scaled(rng, (ny, nx), np.float32)
    cm = contour2d(q, lat, lon, dA)
    lv = np.quantile(q, [0.9, 0.1, 0.5, 0.3, 0.7])                           # in the caller's order, not ascending
    c = {'latitude': lat, 'longitude': lon}
    fields = {'g1': xa.DataArray(g1, ('latitude', 'longitude'), c, 'g1'), 'g2': g2}
    deep = 0
    for side in ('upper', 'lower'):
        out = cm.cal_contour_piece_props(lv, fields=fields, latlon=True, periodic=True, side=side)
        tree, labels = cm.cal_contour_piece_labels(lv, periodic=True, side=side)
        planes = {'g1': g1, 'g2': g2.astype(np.float64)}
        planes.update({'mom%d' % k: p for k, p in enumerate(xa.Contour2D._moment_planes(lat, lon, True, 360.0))})
        for k in range(lv.size):
            t = out[k]
            against_the_map(t, tree[k], labels.values[k], dA, planes, q, lat, lon)
            cy, cx = xa.Contour2D._centroid_of([t['mom0'], t['mom1'], t['mom2']], t['area'], True, 360.0, float(lon[0]))
            assert np.array_equal(t['centroid_y'], cy, equal_nan=True) and np.array_equal(t['centroid_x'], cx, equal_nan=True)
            m0, m1, m2 = t['mom0'], t['mom1'], t['mom2']
            with np.errstate(all='ignore'):
                ok = t['closed'] & ~((m0 == 0) & (m1 == 0) & (m2 == 0))
                assert np.array_equal(t['centroid_y'][ok], np.degrees(np.arctan2(m2, np.hypot(m0, m1)))[ok])
                assert np.array_equal(t['centroid_x'][ok], (np.degrees(np.arctan2(m1, m0)) % 360)[ok])
            deep = max(deep, int(t['depth'].max()) if t.size else 0)
    assert deep >= 1


def test_a_two_slab_stack_with_leading_dims_a_nan_level_and_per_slab_fields():
    ny, nx = 24, 31
    q = np.stack([CS.smooth_noise(ny, nx, 60 + s) for s in range(2)])
    q[1, 5, 7] = np.nan
    y, x = np.linspace(60.0, -60.0, ny), np.arange(nx) * (360.0 / nx)        # descending latitude
    rng = np.random.default_rng(61)
    dA = scaled(rng, (ny, nx))
    cm = contour2d(q, y, x, dA, lead=(('d0', 2),))
    lv = np.array([0.8, np.nan, -0.9, 0.2])
    c = {'d0': np.arange(2), 'latitude': y, 'longitude': x}
    g = scaled(rng, (2, ny, nx))
    e = rng.integers(-2, 3, (2, ny, nx)).astype(np.float64)
    fields = {'g': xa.DataArray(g, ('d0', 'latitude', 'longitude'), c, 'g')}
    ext = xa.DataArray(e, ('d0', 'latitude', 'longitude'), c, 'e')
    out = cm.cal_contour_piece_props(lv, fields=fields, extremum=ext, periodic=360.0)
    tree, labels = cm.cal_contour_piece_labels(lv, periodic=360.0)
    mom = xa.Contour2D._moment_planes(y, x, False, 360.0)
    tied = False
    for s in range(2):
        assert len(out[s]) == 4 and out[s][1].size == 0 and 'centroid_x' in out[s][1].dtype.names
        for k in (0, 2, 3):
            planes = {'g': g[s], 'mom0': mom[0], 'mom1': mom[1], 'mom2': mom[2]}
            t = out[s][k]
            against_the_map(t, tree[s][k], labels.values[s, k], dA, planes, e[s], y, x)
            m = labels.values[s, k]
            tied |= any(((m == p) & (e[s] == t['vmin_net'][p])).sum() > 1 for p in np.flatnonzero(t['closed']))
            ok = t['closed'] & (t['area'] != 0)
            assert np.array_equal(t['centroid_y'][ok], (t['mom0'] / t['area'])[ok])
            assert np.array_equal(t['centroid_x'][ok], ((np.arctan2(t['mom2'], t['mom1']) % (2 * np.pi)) * 360.0 / (2 * np.pi) + x[0])[ok])
    assert tied and any(out[s][k]['depth'].max() > 0 for s in range(2) for k in (0, 2, 3) if out[s][k].size)
    none = cm.cal_contour_piece_props(lv, extremum=False, centroid=False, periodic=360.0)
    assert none[0][0].dtype.names == tree[0][0].dtype.names and none[0][0].tobytes() == tree[0][0].tobytes()


@pytest.mark.parametrize('latlon, periodic', [(True, True), (False, False), (False, 360.0)], ids=['latlon', 'plain', 'periodic'])
def test_the_three_centroid_rows_on_a_small_plane(latlon, periodic):
    ny, nx = 9, 12
    y, x = np.linspace(-40.0, 40.0, ny), np.arange(0.0, 360.0, 30.0)
    q = np.zeros((ny, nx))
    q[3:6, [10, 11, 0, 1] if periodic else [4, 5, 6, 7]] = 1.0               # on a ring: a blob across the seam
    dA = np.cos(np.deg2rad(y))[:, None] * np.ones((ny, nx))
    cm = contour2d(q, y, x, dA)
    (t,) = cm.cal_contour_piece_props(np.array([0.5]), latlon=latlon, periodic=periodic)
    assert t.size == 1 and t['closed'][0] and t['nodes'][0] == 12
    assert ('mom2' in t.dtype.names) == bool(latlon or periodic)
    assert abs(t['centroid_y'][0]) < 1e-9
    want = 345.0 if periodic else 165.0
    assert abs(t['centroid_x'][0] - want) < 1e-9
    assert t['vmin'][0] == 1.0 and t['vmin_y'][0] == y[3] and t['vmin_x'][0] == x[0 if periodic else 4]   # of equal values the smallest flat node


def test_too_many_fields_raise_with_the_numbers():
    ny, nx = 9, 12
    y, x = np.linspace(-40.0, 40.0, ny), np.arange(0.0, 360.0, 30.0)
    q = CS.smooth_noise(ny, nx, 1)
    cm = contour2d(q, y, x, np.ones((ny, nx)))
    fields = {'f%d' % k: np.ones((ny, nx)) for k in range(6)}
    with pytest.raises(Exception, match='6 fields and 3 moment planes are 9'):
        cm.cal_contour_piece_props(np.array([0.0]), fields=fields, latlon=True, periodic=True)
    out = cm.cal_contour_piece_props(np.array([0.0]), fields=fields, periodic=False)     # 6 + 2: as many as one call takes
    assert 'f5_net' in out[0].dtype.names and 'mom1' in out[0].dtype.names and 'mom2' not in out[0].dtype.names
    with pytest.raises(Exception, match='taken'):
        cm.cal_contour_piece_props(np.array([0.0]), fields={'area': np.ones((ny, nx))})
