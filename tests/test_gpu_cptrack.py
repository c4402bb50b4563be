"""Contour2D.cal_contour_piece_tracks (K20 once per step, K22 between steps, K23 over the stack) on the GPU, on the drifting blobs of
cptrack_ref.scene (24 x 48, 12 steps, 3 levels; test_cptrack_host.py shows what the scene holds), against the library's own calls --
the tree is cal_contour_piece_tree's byte for byte, the links of a step are cal_contour_piece_overlap's rows of that pair of steps bit
for bit -- and against cptrack_ref.tracks_of_rows (a union-find in plain Python) run on those rows: every integer equal."""
import numpy as np
import pytest

import cptrack_ref as KR
import xcontour_amd as xa
from test_gpu_cptree import contour2d

pytestmark = pytest.mark.gpu

Y, X = np.linspace(-60.0, 60.0, KR.NY), np.arange(KR.NX) * (360.0 / KR.NX)
DA = np.random.default_rng(2310).random((KR.NY, KR.NX)) + 0.5
NEW = ('track', 'nprev', 'nnext')


def pairs_of(q, periodic):
    """cal_contour_piece_overlap of every pair of consecutive steps -> per step the overlap per level"""
    out = []
    for t in range(q.shape[0] - 1):
        cm = contour2d(q[t], Y, X, DA)
        other = xa.DataArray(q[t + 1], ('latitude', 'longitude'), {'latitude': Y, 'longitude': X}, 'next')
        out.append(cm.cal_contour_piece_overlap(KR.LEVELS, other, periodic=periodic)[2])
    return out


def check(got, k19, pairs, min_overlap, nstep):
    """one series: got = (tree[t][k], links[k], tracks[k])"""
    tree, links, tracks = got
    assert len(tree) == nstep and len(links) == KR.LEVELS.size and len(tracks) == KR.LEVELS.size
    for t in range(nstep):
        for k in range(KR.LEVELS.size):
            a, b = tree[t][k], k19[t][k]
            assert a.dtype.names == b.dtype.names + NEW and a['track'].dtype == np.int64 and a['nprev'].dtype == np.int32
            assert all(a[f].tobytes() == b[f].tobytes() for f in b.dtype.names), 'the tree is not cal_contour_piece_tree\'s'
    for k in range(KR.LEVELS.size):
        lk = links[k]
        assert lk.dtype.names == ('step', 'a', 'b', 'nodes', 'area', 'linked') and lk['step'].dtype == np.int32 and lk['linked'].dtype == np.bool_
        assert np.array_equal(lk, lk[np.lexsort((lk['b'], lk['a'], lk['step']))]), 'sorted by (step, a, b)'
        rows = []
        for t in range(nstep - 1):
            mine, ov = lk[lk['step'] == t], pairs[t][k]
            assert all(mine[f].tobytes() == ov[f].tobytes() for f in ('a', 'b', 'nodes', 'area')), 'step %d level %d' % (t, k)
            rows.append(ov)
        assert lk.size == sum(r.size for r in rows)
        ref = KR.tracks_of_rows([tree[t][k].size for t in range(nstep)], [tree[t][k]['nodes_net'] for t in range(nstep)], rows, min_overlap)
        for t in range(nstep):
            for f in NEW:
                assert np.array_equal(tree[t][k][f], ref[f][t]), (f, t, k)
        assert np.array_equal(lk['linked'], np.concatenate(ref['linked']) if rows else np.empty(0, dtype=bool)), k
        assert tracks[k].dtype == KR.TRACK_DTYPE and np.array_equal(tracks[k], ref['tracks']), k
    return tree, links, tracks


def same(a, b):
    """two nested results equal byte for byte"""
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope='module')
def base():
    """the scene, its tree and its pairwise overlaps, computed once"""
    q = KR.scene()
    cm = contour2d(q, Y, X, DA, lead=(('time', KR.NSTEP),))
    return q, cm, cm.cal_contour_piece_tree(KR.LEVELS, periodic=True), pairs_of(q, True)


@pytest.fixture(scope='module')
def tracked(base):
    q, cm, k19, pairs = base
    return check(cm.cal_contour_piece_tracks(KR.LEVELS, 'time', periodic=True), k19, pairs, 0.0, KR.NSTEP)


def test_the_scene_against_the_tree_the_pairwise_overlaps_and_the_restatement(tracked):
    tree, links, tracks = tracked
    assert any((tk['nmerge'] >= 1).any() for tk in tracks) and any((tk['nsplit'] >= 1).any() for tk in tracks)
    assert any(((tk['nrings'] == 1)).any() for tk in tracks) and any((tk['first_step'] > 0).any() for tk in tracks)
    assert all(lk['linked'].any() and (lk['a'] == -1).any() for lk in links)
    for k in range(KR.LEVELS.size):                                           # first_row names the first ring: its track is the row itself
        for j, tk in enumerate(tracks[k]):
            assert tree[tk['first_step']][k]['track'][tk['first_row']] == j


@pytest.mark.parametrize('steps', [1, 2, 5])
def test_batches_of_one_two_and_five_steps_give_the_same(base, tracked, steps):
    """the carried map and permutation at every batch edge"""
    q, cm, _, _ = base
    per = KR.NY * KR.NX * (q.dtype.itemsize + 4 * KR.LEVELS.size)            # what a step stages: the tracer and its maps (dA is one plane)
    keep = cm.ctx.max_batch_bytes
    try:
        cm.ctx.max_batch_bytes = per * steps
        assert [b - a for a, b in cm.ctx._batches(KR.NSTEP, per)][:2] == [steps, steps]
        got = cm.cal_contour_piece_tracks(KR.LEVELS, 'time', periodic=True)
    finally:
        cm.ctx.max_batch_bytes = keep
    assert same(got, tracked)


def test_min_overlap_a_half(base, tracked):
    q, cm, k19, pairs = base
    _, links, tracks = check(cm.cal_contour_piece_tracks(KR.LEVELS, 'time', periodic=True, min_overlap=0.5), k19, pairs, 0.5, KR.NSTEP)
    assert any((a['linked'] & ~b['linked']).any() for a, b in zip(tracked[1], links)), 'no link that 0.5 rejects and 0 accepts'
    assert sum(t.size for t in tracks) > sum(t.size for t in tracked[2])


@pytest.mark.parametrize('along_first', [False, True], ids=['(member, time)', '(time, member)'])
def test_two_series_along_either_leading_dim(base, tracked, along_first):
    q, _, k19, pairs = base
    q1 = np.ascontiguousarray(q[::-1])                                        # the second series: time reversed, mergers become splits
    one = check(contour2d(q1, Y, X, DA, lead=(('time', KR.NSTEP),)).cal_contour_piece_tracks(KR.LEVELS, 'time', periodic=True),
                [k19[t] for t in range(KR.NSTEP - 1, -1, -1)], pairs_of(q1, True), 0.0, KR.NSTEP)
    both = np.stack([q, q1])
    if along_first:
        cm = contour2d(np.ascontiguousarray(both.transpose(1, 0, 2, 3)), Y, X, DA, lead=(('time', KR.NSTEP), ('member', 2)))
        slab = lambda m, t: t * 2 + m
    else:
        cm = contour2d(both, Y, X, DA, lead=(('member', 2), ('time', KR.NSTEP)))
        slab = lambda m, t: m * KR.NSTEP + t
    tree, links, tracks = cm.cal_contour_piece_tracks(KR.LEVELS, 'time', periodic=True)
    assert len(tree) == 2 * KR.NSTEP and len(links) == 2 and len(tracks) == 2
    for m, ref in enumerate((tracked, one)):
        assert same([tree[slab(m, t)] for t in range(KR.NSTEP)], ref[0]) and same(links[m], ref[1]) and same(tracks[m], ref[2])
    # following the members instead: two steps, twelve series
    t2, l2, k2 = cm.cal_contour_piece_tracks(KR.LEVELS, 'member', periodic=True)
    assert len(l2) == KR.NSTEP and len(k2) == KR.NSTEP and all((lk['step'] == 0).all() for s in l2 for lk in s)
    assert all(a[f].tobytes() == b[f].tobytes() for sa, sb in zip(t2, tree) for a, b in zip(sa, sb) for f in k19[0][0].dtype.names)


def test_a_stack_of_one_step(base):
    q, _, k19, _ = base
    cm = contour2d(q[:1], Y, X, DA, lead=(('time', 1),))
    tree, links, tracks = check(cm.cal_contour_piece_tracks(KR.LEVELS, 'time', periodic=True), k19[:1], [], 0.0, 1)
    for k in range(KR.LEVELS.size):
        n = tree[0][k].size
        assert n > 0 and links[k].size == 0 and tree[0][k]['track'].tolist() == list(range(n)) and not tree[0][k]['nprev'].any()
        assert tracks[k]['nrings'].tolist() == [1] * n and tracks[k]['first_row'].tolist() == list(range(n))


def test_a_plain_plane_has_open_pieces_and_each_is_a_track_of_one(base):
    q, cm, _, _ = base
    tree, links, tracks = check(cm.cal_contour_piece_tracks(KR.LEVELS, 'time', periodic=False),
                                cm.cal_contour_piece_tree(KR.LEVELS, periodic=False), pairs_of(q, False), 0.0, KR.NSTEP)
    opened = 0
    for t in range(KR.NSTEP):
        for k in range(KR.LEVELS.size):
            r = tree[t][k]
            for p in np.flatnonzero(~r['closed']).tolist():
                opened += 1
                assert r['nprev'][p] == 0 and r['nnext'][p] == 0 and tracks[k]['nrings'][r['track'][p]] == 1
    assert opened > 0


def test_along_must_be_a_leading_dim_and_min_overlap_a_fraction(base):
    _, cm, _, _ = base
    for along in ('latitude', 'longitude', 'member', None):
        with pytest.raises(Exception, match='along'):
            cm.cal_contour_piece_tracks(KR.LEVELS, along, periodic=True)
    for mo in (-0.1, 1.5, float('nan')):
        with pytest.raises(Exception, match='min_overlap'):
            cm.cal_contour_piece_tracks(KR.LEVELS, 'time', periodic=True, min_overlap=mo)
