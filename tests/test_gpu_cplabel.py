"""Context.contour_piece_labels and Contour2D.cal_contour_piece_labels (K20) on the GPU, against cplabel_ref.labels_of_masks on
Context.contour_segments of the same input -- every label equal --, and against the library's own kernels: the table is
contour_piece_tree's byte for byte, bincount(labels) is K19's nodes_net, math.fsum over the nodes of a label is K19's area_net and
integral_net bit for bit, and the parity of depth[labels] is K17's select='all' mask."""
import math

import numpy as np
import pytest

import cplabel_ref as LR
import cptree_cases as CS
import cptree_ref as TR
import xcontour_amd as xa
from test_gpu_cpinside_records import scaled
from test_gpu_cptree import contour2d, per_range, reference

pytestmark = pytest.mark.gpu


def against_the_restatement(ctx, q, lv, periodic, flip=False, w=None, f=None):
    pc, tab, lab = ctx.contour_piece_labels(q, lv, w=w, f=f, periodic=periodic, flip=flip)
    nslab, ny, nx = q.shape
    assert lab.dtype == np.int32 and lab.shape == (nslab, len(lv), ny, nx) and tab.dtype == ctx.PIECE_TREE_DTYPE
    pc19, tab19 = ctx.contour_piece_tree(q, lv, w=w, f=f, periodic=periodic, flip=flip)
    assert pc.tobytes() == pc19.tobytes() and tab.tobytes() == tab19.tobytes(), 'the table is not contour_piece_tree\'s'
    ref, masks = reference(ctx, q, lv, periodic, flip, w, f, return_masks=True)
    got = per_range(pc, tab)
    for r, (g, t, ms) in enumerate(zip(got, ref, masks)):
        assert TR.differences(g.astype(TR.DTYPE), t) == [], 'range %d' % r
        m = lab.reshape(-1, ny, nx)[r]
        assert np.array_equal(m, LR.labels_of_masks(ms, (ny, nx))), 'range %d' % r
        assert np.array_equal(np.bincount(m[m >= 0], minlength=g.size)[g['closed']], g['n_net'][g['closed']]), 'range %d' % r
    return pc, tab, lab


@pytest.mark.parametrize('periodic', [False, True], ids=['plain', 'ring'])
def test_three_slabs_both_sides_every_input_kind_and_batches(ctx, periodic):
    ny, nx = 24, 31
    q = np.stack([CS.smooth_noise(ny, nx, 50 + s) for s in range(3)])
    q[2, 5, 7] = np.nan
    lv = np.array([-0.9, -0.3, 0.2, 0.8])
    rng = np.random.default_rng(51)
    w, f = rng.standard_normal((3, ny, nx)), rng.standard_normal((3, ny, nx)).astype(np.float32)
    pc, tab, lab = against_the_restatement(ctx, q, lv, periodic, flip=True, w=w, f=f)
    against_the_restatement(ctx, q, lv, periodic, flip=False, w=w[0], f=f.astype(np.float64))
    against_the_restatement(ctx, q, lv, periodic)
    keep = ctx.max_batch_bytes
    try:
        ctx.max_batch_bytes = 1                                              # one slab per batch
        pc3, tab3, lab3 = ctx.contour_piece_labels(q, lv, w=w, f=f, periodic=periodic, flip=True)
    finally:
        ctx.max_batch_bytes = keep
    assert pc3.tobytes() == pc.tobytes() and tab3.tobytes() == tab.tobytes() and lab3.tobytes() == lab.tobytes()
    assert (tab['depth'] > 0).any() and (~tab['closed']).any() and (lab >= 0).any() and (lab == -1).any()
    pc0, tab0, lab0 = ctx.contour_piece_labels(q, np.array([99.0]), periodic=periodic)     # a level nothing crosses
    assert not pc0.any() and tab0.size == 0 and lab0.shape == (3, 1, ny, nx) and (lab0 == -1).all()


def test_a_resident_tracer(ctx):
    q = CS.stacked_siblings()[None].copy()
    _, tab, lab = against_the_restatement(ctx, q, np.array([0.5]), False)
    ctx.keep_resident(q)
    try:
        _, tab2, lab2 = against_the_restatement(ctx, q, np.array([0.5]), False)
    finally:
        ctx.release_resident(q)
    assert tab2.tobytes() == tab.tobytes() and lab2.tobytes() == lab.tobytes()
    block, upper, lower, island = (int(np.flatnonzero(tab['n_in'] == n)[0]) for n in (98, 20, 9, 1))
    assert lab[0, 0, 5, 3] == island and lab[0, 0, 4, 3] == upper and lab[0, 0, 11, 4] == lower and lab[0, 0, 1, 1] == block
    assert lab[0, 0, 0, 0] == -1 and tab['depth'].max() == 2


def test_descending_levels_an_empty_level_leading_dims_and_the_tree():
    ny, nx = 24, 31
    q = np.stack([CS.smooth_noise(ny, nx, 60 + s) for s in range(2)])
    y, x = np.linspace(-60.0, 60.0, ny), np.arange(nx) * (360.0 / nx)
    dA = np.random.default_rng(61).random((ny, nx)) + 0.5
    cm = contour2d(q, y, x, dA, lead=(('d0', 2),))
    lv = np.array([0.8, 0.2, np.nan, -0.9, 99.0])                             # descending, a NaN level, one nothing crosses
    g = xa.DataArray(q * q, ('d0', 'latitude', 'longitude'), {'d0': np.arange(2), 'latitude': y, 'longitude': x}, 'q2')
    for side in ('upper', 'lower'):
        tree, labels = cm.cal_contour_piece_labels(lv, integrand=g, periodic=True, side=side)
        k19 = cm.cal_contour_piece_tree(lv, integrand=g, periodic=True, side=side)
        assert labels.dims == ('d0', 'contour', 'latitude', 'longitude') and labels.values.dtype == np.int32
        assert np.array_equal(np.asarray(labels.coords['latitude']), y) and np.array_equal(np.asarray(labels.coords['longitude']), x)
        lab = labels.values
        assert lab.shape == (2, 5, ny, nx) and (lab[:, 2] == -1).all() and (lab[:, 4] == -1).all()
        ref, masks = reference(cm.ctx, q, lv[[3, 1, 0]], True, side == 'lower', w=dA, f=q * q, return_masks=True)   # ascending latitude
        for s in range(2):
            assert len(tree[s]) == 5 and tree[s][2].size == 0 and tree[s][4].size == 0
            for k in range(5):
                assert tree[s][k].dtype == k19[s][k].dtype and tree[s][k].tobytes() == k19[s][k].tobytes(), (s, k)
            for j, k in enumerate((3, 1, 0)):
                assert np.array_equal(lab[s, k], LR.labels_of_masks(masks[s * 3 + j], (ny, nx))), (s, k)
                t = tree[s][k]
                m = lab[s, k]
                assert np.array_equal(np.bincount(m[m >= 0], minlength=t.size)[t['closed']], t['nodes_net'][t['closed']])
        assert (lab >= 0).any() and any(tree[s][k].size and tree[s][k]['depth'].max() > 0 for s in range(2) for k in (0, 1, 3))
    with pytest.raises(Exception, match='side'):
        cm.cal_contour_piece_labels(lv, periodic=True, side='north')


@pytest.mark.parametrize('periodic', [False, True], ids=['plain', 'ring'])
def test_the_sums_over_a_label_are_k19s_net_sums_bit_for_bit(periodic):
    """weights and integrands with exponents in [-20, 20]: every term lies inside its window, where DESIGN.md says the rule is plain fsum"""
    ny, nx = 24, 31
    q = CS.smooth_noise(ny, nx, 5)
    y, x = np.linspace(-60.0, 60.0, ny), np.arange(nx) * (360.0 / nx)
    rng = np.random.default_rng(81)
    dA, g = scaled(rng, (ny, nx)), scaled(rng, (ny, nx))
    cm = contour2d(q, y, x, dA)
    lv = np.linspace(-1.5, 1.5, 9)
    gi = xa.DataArray(g, ('latitude', 'longitude'), {'latitude': y, 'longitude': x}, 'g')
    tree, labels = cm.cal_contour_piece_labels(lv, integrand=gi, periodic=periodic)
    lab, rings, deep = labels.values, 0, 0
    for k in range(lv.size):
        t, m = tree[k], lab[k]
        assert np.array_equal(np.bincount(m[m >= 0], minlength=t.size)[t['closed']], t['nodes_net'][t['closed']])
        for p in np.flatnonzero(t['closed']):
            assert math.fsum(dA[m == p]) == t['area_net'][p], (k, p)
            assert math.fsum((dA * g)[m == p]) == t['integral_net'][p], (k, p)
            rings += 1
        deep = max(deep, int(t['depth'].max()) if t.size else 0)
    assert rings > 20 and deep >= 1 and (lab == -1).any()


def test_the_parity_of_the_depths_is_k17s_mask_and_the_threshold():
    """a NaN-free periodic plane whose first and last rows lie below every level: every piece is a closed ring.  Rings that go round
    are among them (the one between row 0 and row 1 always is): without flip their inside set is the parity P_p like every other
    ring's, so a node lies in depth[label] + 1 rings, and K17's select='all' parity is true exactly where that number is odd."""
    ny, nx = 24, 31
    q = CS.smooth_noise(ny, nx, 2)
    q[0] = q[-1] = -10.0
    y, x = np.linspace(-60.0, 60.0, ny), np.arange(nx) * (360.0 / nx)
    cm = contour2d(q, y, x, np.ones((ny, nx)))
    lv = np.linspace(-2.0, 2.0, 20)
    tree, labels = cm.cal_contour_piece_labels(lv, periodic=True)
    every = cm.cal_integral_inside_contours(lv, periodic=True, select='all', side='upper', return_mask=True)['mask'].values
    lab = labels.values
    for k in range(lv.size):
        t, m = tree[k], lab[k]
        assert t['closed'].all()
        even = (m >= 0) & (t['depth'][np.maximum(m, 0)] % 2 == 0) if t.size else np.zeros((ny, nx), dtype=bool)
        assert np.array_equal(even, every[k]), k
        assert np.array_equal(every[k], q > lv[k]), k
    assert max(int(t['depth'].max()) for t in tree if t.size) >= 2 and (lab >= 0).any() and (lab == -1).any()
