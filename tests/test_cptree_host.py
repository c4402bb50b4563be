"""The restatement of K19 (cptree_ref.piece_tree, sets of nodes) and a second, independent one of the kernel's column walk (walk_parents
below), on the CPU -- no GPU.  The records come from the restatements of K12 (contour_join_ref, contour_join_periodic_ref), as in
test_cpinside_host.py.  First the set restatement on the hand-built planes of cptree_cases, answers written out; the walk must give the
same parents on every one of them and on noise; last, three broken walks that each fail the case written for it."""
import numpy as np
import pytest

import contour_join_periodic_ref as JP
import contour_join_ref as JR
import cpinside_ref as PR
import cptree_cases as CS
import cptree_ref as TR

WRONG = ('no skip', 'flip ignored', 'open pieces are rings')


def records(q, periodic, levels=(0.5,)):
    q = np.asarray(q, dtype=np.float64)
    rec = (JP if periodic else JR).stack_records(q[None], np.asarray(levels, dtype=np.float64))
    return rec + q.shape + (1 if periodic else 0,)


def walk_parents(count, e_from, e_to, pts, ny, nx, periodic, flip=0, wrong=None):
    """the kernel's parent walk -> per range the parents (rows in first_edge order, -1 for none).  Per ring: the sign S as in
    cpinside_ref.mapping; the crossing next to its outside node -- the topmost one, or with flip the bottommost one: without flip it is
    row 0 that lies outside every ring, with flip row ny - 1 --; from there away from the ring to that row.  A crossing of another
    ring has that ring's inside below it iff (s == S) != (winding != 0 and flip): inside on the walker's side -> parent; else skip to
    that ring's next crossing."""
    assert wrong is None or wrong in WRONG
    count, ef, et, pts = PR._ranges(count, e_from, e_to, pts)
    wflip = 0 if wrong == 'flip ignored' else flip
    out, s0 = [], 0
    for c in count:
        pcs = sorted(PR._pieces(ef, et, pts, s0, c, ny, nx, periodic), key=lambda t: t[3])
        owner, sign, S, ring = {}, {}, [], []
        for k, (g, closed, wind, _) in enumerate(pcs):
            ring.append(closed or wrong == 'open pieces are rings')
            A = B = 0
            for i in g[(ef[g] & 1) == 1]:
                node = int(ef[i]) >> 1
                row, col = node // nx, node % nx
                if row >= ny - 1:
                    continue
                right = 2 * (row * nx + (col + 1) % nx) + 1
                s = 1 if int(et[i]) in (2 * node, 2 * (node + nx), right) else -1
                owner[(row, col)], sign[(row, col)] = k, s
                A, B = A + s, B + s * row
            S.append(((A > 0) - (A < 0)) if wind != 0 else ((B < 0) - (B > 0)))
        parents = []
        for k, (g, closed, wind, _) in enumerate(pcs):
            mine = sorted(key for key, o in owner.items() if o == k)
            if not closed or not mine:
                parents.append(-1)
                continue
            down = bool(wflip)
            row, col = mine[-1] if down else mine[0]                         # the largest edge id (bottommost), else the smallest
            parent, skip = -1, -1
            edges = range(row + 1, ny - 1) if down else range(row - 1, -1, -1)
            for e in edges:
                x = owner.get((e, col))
                if x is None or not ring[x]:
                    continue
                if skip >= 0:
                    skip = -1 if x == skip else skip
                    continue
                assert x != k, 'the walk met its own ring'
                below = (sign[(e, col)] == S[x]) != (pcs[x][2] != 0 and bool(wflip))
                if below != down:
                    parent = x
                    break
                if wrong != 'no skip':
                    skip = x
            parents.append(parent)
        out.append(np.array(parents, dtype=np.int64))
        s0 += int(c)
    return out


def agree(rec, flip=0, **kw):
    """the walk gives the parents of the set restatement; -> its tables"""
    tables = TR.piece_tree(*rec, flip=flip, **kw)
    for t, p in zip(tables, walk_parents(*rec, flip=flip)):
        assert np.array_equal(t['parent'], p)
    return tables


# ------------------------------------------------------------------ the set restatement on the hand-built planes, and the walk on each
@pytest.mark.parametrize('n', [13, 83])
def test_a_chain_of_square_rings(n):
    (t,) = agree(records(CS.chain(n), False))
    m = (n - 1) // 2
    t = t[np.argsort(t['n_in'])]
    assert t.size == m and t['closed'].all()
    k = np.arange(m)
    assert np.array_equal(t['n_in'], (2 * k + 1) ** 2) and np.array_equal(t['depth'], m - 1 - k)
    assert np.array_equal(t['n_net'], np.where(k > 0, (2 * k + 1) ** 2 - (2 * k - 1) ** 2, 1))
    assert np.array_equal(t['nchild'], (k > 0).astype(np.int32)) and np.array_equal(t['net_w'], t['n_net'].astype(np.float64))


def test_stacked_siblings():
    (t,) = agree(records(CS.stacked_siblings(), False))
    by = {int(n): row for n, row in zip(t['n_in'], t)}
    assert sorted(by) == [1, 9, 20, 98]
    block, upper, lower, island = (int(np.flatnonzero(t['n_in'] == n)[0]) for n in (98, 20, 9, 1))
    assert t['parent'].tolist()[block] == -1 and t['parent'][upper] == block and t['parent'][lower] == block and t['parent'][island] == upper
    assert t['nchild'][block] == 2 and t['nchild'][upper] == 1 and t['depth'][island] == 2
    assert t['n_net'][block] == 98 - 20 - 9 and t['n_net'][upper] == 19


def test_two_unrelated_blobs_one_above_the_other():
    (t,) = agree(records(CS.two_blobs(), False))
    assert t['parent'].tolist() == [-1, -1] and t['depth'].tolist() == [0, 0] and np.array_equal(t['n_net'], t['n_in'])


@pytest.mark.parametrize('flip', [0, 1])
def test_two_rings_that_go_round_and_three_blobs(flip):
    q = CS.bands()
    (t,) = agree(records(q, True), flip=flip)
    assert t.size == 5 and sorted(np.abs(t['winding']).tolist()) == [0, 0, 0, 1, 1]
    above, upper, between, lower, below = range(5)                          # first_edge order: rows 0/1, 2, 3/4, 5, 6/7
    assert t['winding'][upper] != 0 and t['winding'][lower] != 0
    want = [-1, -1, upper, upper, lower] if not flip else [upper, lower, lower, -1, -1]
    assert t['parent'].tolist() == want
    assert t['n_in'][upper] == (48 if not flip else 24) and t['n_in'][lower] == (24 if not flip else 48)


def test_a_ring_across_the_seam_and_the_same_field_on_a_plain_plane():
    (t,) = agree(records(CS.seam(), True))
    assert t.size == 3 and t['closed'].all() and (t['winding'] == 0).all()
    t = t[np.argsort(-t['n_in'])]
    assert t['n_in'].tolist() == [42, 9, 1] and t['depth'].tolist() == [0, 1, 2] and t['n_net'].tolist() == [33, 8, 1]
    (p,) = agree(records(CS.seam(), False))
    assert not p['closed'].any() and (p['parent'] == -1).all() and (p['n_net'] == -1).all() and np.isnan(p['net_w']).all()


@pytest.mark.parametrize('q', [CS.open_above(), CS.open_beside_nan(False)], ids=['edge to edge', 'beside a NaN cell'])
def test_an_open_piece_above_a_ring_is_transparent(q):
    (t,) = agree(records(q, False))
    assert sorted(t['closed'].tolist()) == [False, True]
    o, r = t[~t['closed']][0], t[t['closed']][0]
    assert r['parent'] == -1 and r['n_in'] == 1 and r['n_net'] == 1
    assert (o['parent'], o['depth'], o['nchild'], o['n_net']) == (-1, 0, 0, -1) and np.isnan(o['net_w']) and np.isnan(o['net_wf'])


def test_saddles_and_a_single_node():
    (t,) = agree(records(CS.checkerboard(), False))
    assert t.size >= 4
    (t,) = agree(records(CS.one_node(), False))
    assert t['parent'].tolist() == [-1] and t['n_net'].tolist() == [1]


def test_a_long_walk():
    (t,) = agree(records(CS.long_walk(True), True))
    assert sorted(t['n_in'].tolist()) == [1, 3 * 598] and t['parent'][np.argmin(t['n_in'])] == np.argmax(t['n_in'])
    (t,) = agree(records(CS.long_walk(False), True))
    assert t['parent'].tolist() == [-1]


@pytest.mark.parametrize('periodic', [False, True], ids=['plain', 'ring'])
@pytest.mark.parametrize('seed', [1, 2, 3])
def test_the_walk_is_the_set_rule_on_smooth_noise(seed, periodic):
    q = CS.smooth_noise(24, 31, seed)
    q[5, 7] = np.nan
    lv = np.linspace(-1.8, 1.8, 13)
    w = np.random.default_rng(seed).standard_normal((24, 31))
    deep = 0
    for flip in (0, 1):
        tables = agree(records(q, periodic, lv), flip=flip, w=w)
        deep = max(deep, max(int(t['depth'].max()) for t in tables if t.size))
        for t in tables:                                                      # the children's sets are disjoint subsets
            kids = np.zeros(t.size, dtype=np.int64)
            np.add.at(kids, t['parent'][t['parent'] >= 0], t['n_in'][t['parent'] >= 0])
            assert np.array_equal(t['n_net'][t['closed']], (t['n_in'] - kids)[t['closed']])
    assert deep >= (2 if periodic else 1)


# ------------------------------------------------------------------ three broken walks, each caught by its case
def caught(rec, wrong, flip=0):
    tables = TR.piece_tree(*rec, flip=flip)
    try:
        return any(not np.array_equal(t['parent'], p) for t, p in zip(tables, walk_parents(*rec, flip=flip, wrong=wrong)))
    except AssertionError:                                                   # the walk met its own ring
        return True


def test_a_walk_without_the_skip_rule_is_caught_by_the_stacked_siblings():
    assert caught(records(CS.stacked_siblings(), False), 'no skip')
    assert not caught(records(CS.chain(13), False), 'no skip')               # a chain cannot tell


def test_a_walk_that_ignores_flip_is_caught_by_the_two_rings_that_go_round():
    assert caught(records(CS.bands(), True), 'flip ignored', flip=1)
    assert not caught(records(CS.bands(), True), 'flip ignored', flip=0)


def test_a_walk_that_takes_open_pieces_for_rings_is_caught():
    assert caught(records(CS.open_beside_nan(True), False), 'open pieces are rings')
    (t,) = agree(records(CS.open_beside_nan(True), False))
    hole = t[t['closed'] & (t['n_in'] == 1)][0]
    assert hole['parent'] == int(np.argmax(t['n_in'])) and hole['depth'] == 1   # its parent lies BEHIND the open piece
