"""Context.contour_piece_tree and Contour2D.cal_contour_piece_tree (K19) on the GPU, against cptree_ref.piece_tree on
Context.contour_segments of the same input -- integers equal, sums bit for bit -- and against the library's own K13, K17 and K18: the rows
line up with cal_contour_pieces, K18's fields are cal_integral_inside_pieces', and the depths give the parity of K17's select='all' mask."""
import numpy as np
import pytest

import cptree_cases as CS
import cptree_ref as TR
import xcontour_amd as xa

pytestmark = pytest.mark.gpu

NET = {'n_in': 'nodes', 'sum_w': 'area', 'sum_wf': 'integral', 'n_net': 'nodes_net', 'net_w': 'area_net', 'net_wf': 'integral_net'}


def per_range(pc, table):
    off = np.concatenate([[0], np.cumsum(pc.ravel().astype(np.int64))])
    return [table[a:b] for a, b in zip(off[:-1], off[1:])]


def reference(ctx, q, lv, periodic, flip, w=None, f=None, return_masks=False):
    cnt, ef, et, pts = ctx.contour_segments(q, lv, periodic=periodic)
    return TR.piece_tree(cnt.ravel(), ef, et, pts, q.shape[1], q.shape[2], int(periodic), flip=int(flip), ncont=len(lv), w=w, f=f,
                         return_masks=return_masks)


def against_the_restatement(ctx, q, lv, periodic, flip=False, w=None, f=None):
    pc, tab = ctx.contour_piece_tree(q, lv, w=w, f=f, periodic=periodic, flip=flip)
    assert tab.dtype == ctx.PIECE_TREE_DTYPE and pc.shape == (q.shape[0], len(lv))
    ref, got = reference(ctx, q, lv, periodic, flip, w, f), per_range(pc, tab)
    assert [g.size for g in got] == [t.size for t in ref]
    for r, (g, t) in enumerate(zip(got, ref)):
        assert TR.differences(g.astype(TR.DTYPE), t) == [], 'range %d' % r
    return pc, tab, got


def contour2d(q, y, x, dA, lead=()):
    c = {'latitude': y, 'longitude': x}
    c.update({d: np.arange(n) for d, n in lead})
    dims = tuple(d for d, _ in lead) + ('latitude', 'longitude')
    return xa.Contour2D(xa.DataArray(q, dims, c, 'q'), xa.DataArray(dA, ('latitude', 'longitude'), c, 'dA'),
                        {'X': 'longitude', 'Y': 'latitude'}, {'Y': 'latitude'}, dtype=np.float64)


def as_ref(rows, has_f):
    """a facade array under the restatement's names"""
    t = np.empty(rows.size, dtype=TR.DTYPE)
    back = {v: k for k, v in NET.items()}
    for name in rows.dtype.names:
        t[back.get(name, name)] = rows[name]
    if not has_f:
        t['sum_wf'], t['net_wf'] = np.nan, np.nan
    return t


@pytest.mark.parametrize('periodic', [False, True], ids=['plain', 'ring'])
def test_three_slabs_every_input_kind_batches_and_k18s_fields(ctx, periodic):
    ny, nx = 24, 31
    q = np.stack([CS.smooth_noise(ny, nx, 50 + s) for s in range(3)])
    q[2, 5, 7] = np.nan
    lv = np.array([-0.9, -0.3, 0.2, 0.8])
    rng = np.random.default_rng(51)
    w, f = rng.standard_normal((3, ny, nx)), rng.standard_normal((3, ny, nx)).astype(np.float32)
    pc, tab, got = against_the_restatement(ctx, q, lv, periodic, flip=True, w=w, f=f)
    against_the_restatement(ctx, q, lv, periodic, flip=False, w=w[0], f=f.astype(np.float64))
    against_the_restatement(ctx, q, lv, periodic)
    keep = ctx.max_batch_bytes
    try:
        ctx.max_batch_bytes = 1                                              # one slab per batch
        pc3, tab3 = ctx.contour_piece_tree(q, lv, w=w, f=f, periodic=periodic, flip=True)
    finally:
        ctx.max_batch_bytes = keep
    assert pc3.tobytes() == pc.tobytes() and tab3.tobytes() == tab.tobytes()
    pc18, tab18 = ctx.contour_piece_interiors(q, lv, w=w, f=f, periodic=periodic, flip=True)
    assert np.array_equal(pc, pc18)
    for k in tab18.dtype.names:
        assert tab[k].tobytes() == tab18[k].tobytes(), k
    assert (tab['depth'] > 0).any() and (~tab['closed']).any()
    assert ctx.contour_piece_tree(q, np.array([99.0]))[1].size == 0


def test_the_chains_in_closed_form(ctx):
    for n in (13, 83):
        _, tab, _ = against_the_restatement(ctx, CS.chain(n)[None], np.array([0.5]), False)
        m = (n - 1) // 2
        t = tab[np.argsort(tab['n_in'])]
        k = np.arange(m)
        assert np.array_equal(t['n_in'], (2 * k + 1) ** 2) and np.array_equal(t['depth'], m - 1 - k)
        assert np.array_equal(t['n_net'], np.where(k > 0, (2 * k + 1) ** 2 - (2 * k - 1) ** 2, 1))
        inner = tab['parent'] >= 0                                            # the parent of ring k is ring k + 1
        assert inner.sum() == m - 1 and tab['parent'][np.argmax(tab['n_in'])] == -1
        assert np.array_equal(tab['n_in'][tab['parent'][inner]], (np.sqrt(tab['n_in'][inner]).astype(np.int64) + 2) ** 2)


@pytest.mark.parametrize('ascending', [True, False], ids=['ascending', 'descending'])
def test_two_rings_that_go_round_reverse_with_side(ascending):
    q = CS.bands()
    y, x = np.arange(9) * 2.0 - 8.0, np.arange(8) * 45.0
    cm = contour2d(q, y if ascending else y[::-1].copy(), x, np.ones((9, 8)))
    for side in ('upper', 'lower'):
        (t,) = cm.cal_contour_piece_tree(np.array([0.5]), periodic=True, side=side)
        flip = (side == 'upper') != ascending
        assert t.dtype.names == ('first_edge', 'nseg', 'closed', 'winding', 'nodes', 'area', 'parent', 'depth', 'nchild', 'nodes_net',
                                 'area_net')
        assert t['parent'].tolist() == ([-1, -1, 1, 1, 3] if not flip else [1, 3, 3, -1, -1])
        assert t['nodes'].tolist() == ([1, 48, 1, 24, 1] if not flip else [1, 24, 1, 48, 1])
        assert t['nodes_net'].tolist() == [1, 23, 1, 23, 1]                   # either way: 48 - 24 - 1 and 24 - 1
        assert np.array_equal(t['area_net'], t['nodes_net'].astype(np.float64))
    with pytest.raises(Exception, match='side'):
        cm.cal_contour_piece_tree(np.array([0.5]), periodic=True, side='north')


def test_unsorted_levels_a_nan_level_an_empty_level_and_leading_dims():
    ny, nx = 24, 31
    q = np.stack([CS.smooth_noise(ny, nx, 60 + s) for s in range(2)])
    y, x = np.linspace(-60.0, 60.0, ny), np.arange(nx) * (360.0 / nx)
    rng = np.random.default_rng(61)
    dA = rng.random((ny, nx)) + 0.5
    cm = contour2d(q, y, x, dA, lead=(('d0', 2),))
    lv = np.array([0.8, np.nan, -0.9, 99.0, 0.2])
    g = xa.DataArray(q * q, ('d0', 'latitude', 'longitude'), {'d0': np.arange(2), 'latitude': y, 'longitude': x}, 'q2')
    out = cm.cal_contour_piece_tree(lv, integrand=g, periodic=True)
    k18 = cm.cal_integral_inside_pieces(lv, integrand=g, periodic=True)
    k13 = cm.cal_contour_pieces(lv, periodic=360.0)
    assert len(out) == 2 and all(len(o) == 5 and o[1].size == 0 and o[3].size == 0 for o in out)
    assert out[0][0].dtype.names == ('first_edge', 'nseg', 'closed', 'winding', 'nodes', 'area', 'integral', 'parent', 'depth', 'nchild',
                                     'nodes_net', 'area_net', 'integral_net')
    order = [2, 4, 0]                                                        # the finite levels with segments, ascending
    ref = reference(cm.ctx, q, lv[order], True, False, w=dA, f=q * q)       # ascending latitude, side='upper': no flip
    for s in range(2):
        for j, k in enumerate(order):
            a = out[s][k]
            for name in k18[s][k].dtype.names:
                assert a[name].tobytes() == k18[s][k][name].tobytes(), name
            for name in ('first_edge', 'nseg', 'closed', 'winding'):
                assert np.array_equal(a[name], k13[s][k][name]), name
            assert TR.differences(as_ref(a, True), ref[s * 3 + j]) == [], (s, k)
    bare = cm.cal_contour_piece_tree(lv, periodic=True, side='lower')
    assert 'integral_net' not in bare[0][0].dtype.names and bare[0][0].size == out[0][0].size


@pytest.mark.parametrize('periodic', [False, True], ids=['plain', 'ring'])
@pytest.mark.parametrize('seed', [1, 2, 3])
def test_forty_levels_of_smooth_noise_against_the_sets_and_against_k17s_mask(seed, periodic):
    """the field as it is (open pieces at the free edges at every level) against the sets; then the same field inside a frame far below
    every level, so that every piece is a ring, also against K17"""
    ny, nx = 24, 31
    y, x = np.linspace(-60.0, 60.0, ny), np.arange(nx) * (360.0 / nx)
    dA = np.random.default_rng(70 + seed).standard_normal((ny, nx))          # negative weights among them
    lv = np.linspace(-2.0, 2.0, 40)
    raw = CS.smooth_noise(ny, nx, seed)
    framed = raw.copy()
    framed[0] = framed[-1] = -10.0
    if not periodic:
        framed[:, 0] = framed[:, -1] = -10.0
    for q in (raw, framed):
        cm = contour2d(q, y, x, dA)
        out = cm.cal_contour_piece_tree(lv, periodic=periodic)               # ascending latitude, side='upper': no flip
        ref, masks = reference(cm.ctx, q[None], lv, periodic, False, w=dA, return_masks=True)
        for k in range(40):
            assert TR.differences(as_ref(out[k], False), ref[k]) == [], k
    assert all(t['closed'].all() for t in out), 'the frame left an open piece'
    # K17's select='all' mask is the XOR of every ring's inside set: a node in the net set of ring p lies inside depth[p] + 1 rings
    every = cm.cal_integral_inside_contours(lv, periodic=periodic, select='all', return_mask=True)['mask'].values
    for k in range(40):
        t = out[k]
        seen = np.zeros((ny, nx), dtype=bool)
        for p, m in enumerate(masks[k]):
            net = m.copy()
            for c in np.flatnonzero(t['parent'] == p):
                net &= ~masks[k][c]
            assert net.sum() == t['nodes_net'][p]
            assert (every[k][net] == bool((t['depth'][p] + 1) % 2)).all(), (k, p)
            seen |= net
        assert not every[k][~seen].any()
    assert max(int(t['depth'].max()) for t in out if t.size) >= 2
