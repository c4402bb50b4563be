"""Contour2D.cal_contour_piece_overlap, Context.contour_piece_overlap and xc.label_overlap (K22) on the GPU, against
cpoverlap_ref.overlap_of_maps (np.unique over the pairs, math.fsum of the terms) applied to the two maps of cal_contour_piece_labels --
integers equal, sums bit for bit --, and against the library's own kernels: the two trees are cal_contour_piece_tree's byte for byte and
the rows of a ring add up to K19's nodes_net."""
import numpy as np
import pytest

import cpoverlap_ref as OR
import cptree_cases as CS
import xcontour_amd as xa
from test_gpu_cptree import contour2d

pytestmark = pytest.mark.gpu


def as_ref(ov):
    t = np.empty(ov.size, dtype=OR.DTYPE)
    for k, name in (('a', 'a'), ('b', 'b'), ('n', 'nodes'), ('sum_w', 'area'), ('sum_wf', 'integral')):
        t[k] = ov[name]
    return t


def check_level(ov, ta, tb, ma, mb, dA, g, where):
    assert ov.dtype.names == ('a', 'b', 'nodes', 'area', 'integral') and ov['a'].dtype == np.int32 and ov['nodes'].dtype == np.int64
    assert OR.same(as_ref(ov), OR.overlap_of_maps(ma, mb, dA, g)), where
    for key, t in (('a', ta), ('b', tb)):
        for p in np.flatnonzero(t['closed']).tolist():
            assert ov['nodes'][ov[key] == p].sum() == t['nodes_net'][p], (where, key, p)
        assert ov[key].max(initial=-1) < max(t.size, 1)


def same_trees(got, ref):
    return len(got) == len(ref) and all(a.dtype == b.dtype and a.tobytes() == b.tobytes() for a, b in zip(got, ref))


def test_the_barotropic_field_against_itself_rolled_by_five_columns(baro):
    q, lat, lon = baro
    ny, nx = q.shape
    qb = np.roll(q, 5, axis=1)
    dA = np.cos(np.deg2rad(lat.astype(np.float64)))[:, None] * np.ones(nx) + 0.1
    cm = contour2d(q, lat, lon, dA)
    c = {'latitude': lat, 'longitude': lon}
    other = xa.DataArray(qb, ('latitude', 'longitude'), c, 'qb')
    g = xa.DataArray(q, ('latitude', 'longitude'), c, 'g')
    lv = np.quantile(q.astype(np.float64), [0.1, 0.3, 0.5, 0.7, 0.9])
    tree_a, tree_b, ov = cm.cal_contour_piece_overlap(lv, other, integrand=g, periodic=True)
    assert same_trees(tree_a, cm.cal_contour_piece_tree(lv, integrand=g, periodic=True))
    assert same_trees(tree_b, cm.cal_contour_piece_tree(lv, tracer=other, integrand=g, periodic=True))
    la = cm.cal_contour_piece_labels(lv, integrand=g, periodic=True)[1].values
    lb = cm.cal_contour_piece_labels(lv, tracer=other, integrand=g, periodic=True)[1].values
    for k in range(lv.size):
        check_level(ov[k], tree_a[k], tree_b[k], la[k], lb[k], dA, q, k)
    assert sum(o.size for o in ov) > 20 and any((o['a'] == -1).any() for o in ov) and any((o['b'] == -1).any() for o in ov)
    # the tracer against itself: a diagonal, every ring whole
    tree_a2, tree_b2, ov2 = cm.cal_contour_piece_overlap(lv, cm.tracer, integrand=g, periodic=True)
    assert same_trees(tree_a2, tree_a) and same_trees(tree_b2, tree_a)
    for k in range(lv.size):
        o, t = ov2[k], tree_a[k]
        assert (o['a'] == o['b']).all() and (o['a'] >= 0).all()
        assert np.array_equal(o['nodes'], t['nodes_net'][o['a']]) and np.array_equal(o['area'], t['area_net'][o['a']])
        assert np.array_equal(o['integral'], t['integral_net'][o['a']])
        assert np.array_equal(o['a'], np.flatnonzero(t['closed'] & (t['nodes_net'] > 0)))
    # the maps, downloaded, through the module-level call: the same rows
    pc, rows = xa.label_overlap(la[None], lb[None], w=dA, f=q[None])
    assert pc.shape == (1, 5) and pc[0].tolist() == [o.size for o in ov]
    assert OR.same(rows, np.concatenate([as_ref(o) for o in ov]))


@pytest.mark.parametrize('periodic, side', [(True, 'lower'), (False, 'upper')], ids=['ring, lower', 'plain, upper'])
def test_two_slabs_a_nan_level_descending_levels_and_batches(periodic, side):
    ny, nx = 24, 31
    q = np.stack([CS.smooth_noise(ny, nx, 70 + s) for s in range(2)])
    qb = np.stack([CS.smooth_noise(ny, nx, 70 + s) + 0.3 * CS.smooth_noise(ny, nx, 80 + s) for s in range(2)])
    y, x = np.linspace(-60.0, 60.0, ny), np.arange(nx) * (360.0 / nx)
    dA = np.random.default_rng(71).random((ny, nx)) + 0.5
    cm = contour2d(q, y, x, dA, lead=(('d0', 2),))
    c = {'d0': np.arange(2), 'latitude': y, 'longitude': x}
    other = xa.DataArray(qb, ('d0', 'latitude', 'longitude'), c, 'qb')
    gv = OR.scaled(np.random.default_rng(72), (2, ny, nx), np.float32)
    g = xa.DataArray(gv, ('d0', 'latitude', 'longitude'), c, 'g')
    lv = np.array([0.8, 0.2, np.nan, -0.9, 99.0])                             # descending, a NaN level, one nothing crosses
    lvb = np.array([0.7, 0.3, np.nan, -0.8, 98.0])
    for integrand in (g, None):
        kw = dict(integrand=integrand, periodic=periodic, side=side)
        tree_a, tree_b, ov = cm.cal_contour_piece_overlap(lv, other, other_contours=lvb, **kw)
        ka, la = cm.cal_contour_piece_labels(lv, **kw)
        kb, lb = cm.cal_contour_piece_labels(lvb, tracer=other, **kw)
        for s in range(2):
            assert same_trees(tree_a[s], ka[s]) and same_trees(tree_b[s], kb[s])
            assert ov[s][2].size == 0 and ov[s][4].size == 0
            for k in range(5):
                check_level(ov[s][k], tree_a[s][k], tree_b[s][k], la.values[s, k], lb.values[s, k], dA,
                            None if integrand is None else gv[s], (s, k))
                assert np.isnan(ov[s][k]['integral']).all() == (integrand is None) or ov[s][k].size == 0
        assert sum(ov[s][k].size for s in range(2) for k in range(5)) > 20
    # one slab per batch: the same
    keep = cm.ctx.max_batch_bytes
    try:
        cm.ctx.max_batch_bytes = 1
        tree_a1, tree_b1, ov1 = cm.cal_contour_piece_overlap(lv, other, other_contours=lvb, **kw)
    finally:
        cm.ctx.max_batch_bytes = keep
    for s in range(2):
        assert same_trees(tree_a1[s], tree_a[s]) and same_trees(tree_b1[s], tree_b[s]) and same_trees(ov1[s], ov[s])
    # the maps, downloaded, through the module-level call: (nslab, N, ny, nx) maps, the levels where the caller put them
    pc, rows = xa.label_overlap(la.values, lb.values, w=dA)
    assert pc.shape == (2, 5) and pc.tolist() == [[ov[s][k].size for k in range(5)] for s in range(2)]
    assert OR.same(rows, np.concatenate([as_ref(ov[s][k]) for s in range(2) for k in range(5)]))
    with pytest.raises(Exception, match='other_contours'):
        cm.cal_contour_piece_overlap(lv, other, other_contours=lvb[::-1].copy(), periodic=periodic, side=side)
    with pytest.raises(Exception):                                           # a field without the tracer's leading dim
        cm.cal_contour_piece_overlap(lv, xa.DataArray(qb[0], ('latitude', 'longitude'), {'latitude': y, 'longitude': x}, 'qb'))


def test_the_context_call_keeps_the_tables_of_contour_piece_tree(ctx):
    ny, nx = 24, 31
    qa = np.stack([CS.smooth_noise(ny, nx, 90 + s) for s in range(3)])
    qb = np.roll(qa, 2, axis=2)
    lv = np.array([-0.6, 0.0, 0.5])
    rng = np.random.default_rng(91)
    w, f = OR.scaled(rng, (3, ny, nx)), OR.scaled(rng, (3, ny, nx))
    pa, ta, pb, tb, pc, rows = ctx.contour_piece_overlap(qa, qb, lv, w=w, f=f, periodic=True, flip=True)
    for q, p, t in ((qa, pa, ta), (qb, pb, tb)):
        p19, t19 = ctx.contour_piece_tree(q, lv, w=w, f=f, periodic=True, flip=True)
        assert p.tobytes() == p19.tobytes() and t.tobytes() == t19.tobytes()
    la = ctx.contour_piece_labels(qa, lv, w=w, f=f, periodic=True, flip=True)[2]
    lb = ctx.contour_piece_labels(qb, lv, w=w, f=f, periodic=True, flip=True)[2]
    assert rows.dtype == ctx.OVERLAP_DTYPE and pc.shape == (3, 3)
    ref = [OR.overlap_of_maps(la[s, k], lb[s, k], w[s], f[s]) for s in range(3) for k in range(3)]
    assert pc.ravel().tolist() == [t.size for t in ref] and OR.same(rows, np.concatenate(ref))
    prof = ctx.last_cpoverlap_profile()
    assert prof['groups'] == 1 and prof['rounds'] == 0
