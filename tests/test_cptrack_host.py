"""K23's restatements on the CPU -- no GPU.  cptrack_ref.tracks_of (a union-find over the accepted links) on hand cases with the answers
written out; cptrack_ref.rounds_of (the kernels' hook / compress rounds) reaches the same roots on every case of the GPU record test;
each of four deliberately broken variants is caught by at least one of those cases; and the scene of the facade test, built through
cplabel_ref and cpoverlap_ref, HAS what that test is there to show: a merger, a split, a track across the periodic seam, a track of one
ring, a ring born after step 0 and a link that min_overlap = 0.5 rejects."""
import numpy as np
import pytest

import cplabel_ref as LR
import cpoverlap_ref as OR
import cptrack_ref as KR
import cptree_ref as TR
from test_cptree_host import records

CASES = KR.cases()
SMALL = [name for name in CASES if not name.startswith('100 000')]


def run(c, broken=None, root=None):
    return KR.tracks_of(c['nring'], c['step'], c['size'], c['la'], c['lb'], c['ln'], c['mo'], broken=broken, root=root)


# ------------------------------------------------------------------ the rule, answers written out
def test_the_diamond_written_out():
    t = run(CASES['diamond'])
    assert t['root'].tolist() == [0, 0, 0, 0, 4] and t['track'].tolist() == [0, 0, 0, 0, 1]
    assert t['nprev'].tolist() == [0, 1, 1, 2, 0] and t['nnext'].tolist() == [2, 1, 1, 0, 0] and t['link_ok'].all()
    assert t['rows'].tolist() == [(0, 0, 2, 4, 1, 1), (4, 2, 2, 1, 0, 0)]


def test_two_chains_that_meet_at_their_last_rings_are_one_track_rooted_in_ring_0():
    t = run(CASES['two chains that meet at their last rings'])
    assert (t['root'] == 0).all() and t['rows'].tolist() == [(0, 0, 150, 301, 0, 1)]


def test_duplicates_minus_ones_and_empty_links_written_out():
    t = run(CASES['duplicate links'])
    assert t['nnext'].tolist() == [3, 0, 2, 0] and t['nprev'].tolist() == [0, 3, 0, 2] and t['root'].tolist() == [0, 0, 2, 2]
    assert t['rows'][['nsplit', 'nmerge']].tolist() == [(1, 1), (1, 1)]
    t = run(CASES['-1 on either side'])
    assert t['link_ok'].tolist() == [False, False, False, True, False] and t['root'].tolist() == [0, 1, 2, 2, 4]
    assert t['track'].tolist() == [0, 1, 2, 2, 3] and t['nprev'].sum() == 1
    t = run(CASES['n == 0'])
    assert t['link_ok'].tolist() == [False, True, False] and t['root'].tolist() == [0, 1, 2, 2]


def test_the_threshold_written_out():
    t = run(CASES['the threshold met exactly and missed by one'])
    assert t['link_ok'].tolist() == [True, False, True, False]
    t = run(CASES['the threshold is one rounded product'])
    assert 0.07 * 100.0 > 7.0 and t['link_ok'].tolist() == [False, True]
    assert run(CASES['min_overlap 1'])['link_ok'].tolist() == [True, False]
    c = CASES['no sizes, min_overlap 0']
    assert c['size'] is None and run(c)['track'].tolist() == [0, 0, 0, 1, 1, 2]


def test_what_the_cases_hold():
    assert CASES['one ring, no link']['la'].size == 0
    for order in ('ascending', 'reversed', 'shuffled'):
        t = run(CASES['chain of 5000, %s' % order])
        assert (t['root'] == 0).all() and t['rows'].tolist() == [(0, 0, 4999, 5000, 0, 0)]
    big = CASES['100 000 rings, 150 000 links']
    t = run(big)
    assert big['nring'] == 100000 and big['la'].size == 150000 and 100 < t['rows'].size < 90000
    assert 0 < t['link_ok'].sum() < 150000 and t['rows']['nsplit'].sum() > 0 and t['rows']['nmerge'].sum() > 0
    for nring in (255, 256, 257):
        for nlink in (1, 255, 257):
            c = CASES['%d rings, %d links' % (nring, nlink)]
            assert c['nring'] == nring and c['la'].size == nlink


# ------------------------------------------------------------------ the kernels' rounds reach the rule's roots
@pytest.mark.parametrize('name', SMALL)
def test_the_rounds_reach_the_roots_of_the_union_find(name):
    c = CASES[name]
    ref = run(c)
    root, rounds = KR.rounds_of(c['nring'], c['la'], c['lb'], ref['link_ok'])
    assert np.array_equal(root, ref['root']) and rounds <= c['nring'] + 1
    assert KR.same(run(c, root=root), ref)
    # any link order: the same words
    p = np.random.default_rng(7).permutation(c['la'].size)
    d = dict(c, la=c['la'][p], lb=c['lb'][p], ln=c['ln'][p])
    again = run(d)
    assert np.array_equal(again['root'], ref['root']) and np.array_equal(again['rows'], ref['rows'])
    assert np.array_equal(again['link_ok'], ref['link_ok'][p])


@pytest.mark.parametrize('broken', KR.BROKEN)
def test_every_broken_variant_is_caught_by_a_case_of_the_gpu_record_test(broken):
    caught = []
    for name in SMALL:
        c = CASES[name]
        ref = run(c)
        ok = KR.accepted(c['size'], c['la'], c['lb'], c['ln'], c['mo'], broken)
        root, _ = KR.rounds_of(c['nring'], c['la'], c['lb'], ok, broken)
        if not KR.same(run(c, broken=broken, root=root), ref):
            caught.append(name)
    assert caught, 'no case catches %r' % broken
    expect = {'no compression': 'chain of 5000, ascending', 'smaller root under the larger': 'diamond',
              'threshold > instead of >=': 'the threshold met exactly and missed by one', 'degrees counted on rejected links': 'n == 0'}
    assert expect[broken] in caught


# ------------------------------------------------------------------ the scene of the facade test has what that test is there to show
def scene_graph(min_overlap):
    """-> per level (tables per step, labels per step, K22's rows per pair of steps, cptrack_ref.tracks_of_rows of them)"""
    q = KR.scene()
    tables, labels = [], []
    for t in range(KR.NSTEP):
        tb, masks = TR.piece_tree(*records(q[t], True, KR.LEVELS), return_masks=True)
        tables.append(tb)
        labels.append([LR.labels_of_masks(ms, (KR.NY, KR.NX)) for ms in masks])
    out = []
    for k in range(KR.LEVELS.size):
        rows = [OR.overlap_of_maps(labels[t][k], labels[t + 1][k]) for t in range(KR.NSTEP - 1)]
        tr = KR.tracks_of_rows([tables[t][k].size for t in range(KR.NSTEP)], [tables[t][k]['n_net'] for t in range(KR.NSTEP)], rows,
                               min_overlap)
        out.append(([tables[t][k] for t in range(KR.NSTEP)], [labels[t][k] for t in range(KR.NSTEP)], rows, tr))
    return out


def test_the_scene_has_a_merger_a_split_a_seam_track_a_single_ring_a_late_birth_and_a_weak_link():
    q = KR.scene()
    assert q.shape == (12, 24, 48) and (q[:, 0] < KR.LEVELS.min()).all() and (q[:, -1] < KR.LEVELS.min()).all()
    loose, tight = scene_graph(0.0), scene_graph(0.5)
    merged = split = seam = single = born = weak = False
    for (tables, labels, rows, tr), (_, _, _, tr5) in zip(loose, tight):
        assert all(t['closed'].all() for t in tables)
        tk = tr['tracks']
        merged |= bool((tk['nmerge'] >= 1).any())
        split |= bool((tk['nsplit'] >= 1).any())
        single |= bool(((tk['nrings'] == 1) & (tk['first_step'] == tk['last_step'])).any())
        born |= bool((tk['first_step'] > 0).any())
        for t in range(KR.NSTEP):
            lab = labels[t]
            both = np.intersect1d(lab[:, 0][lab[:, 0] >= 0], lab[:, -1][lab[:, -1] >= 0])        # rings with nodes in columns 0 and 47
            seam |= any(tk['nrings'][tr['track'][t][p]] > 1 for p in both.tolist())
        weak |= any(bool((a & ~b).any()) for a, b in zip(tr['linked'], tr5['linked']))
        assert all(not (b & ~a).any() for a, b in zip(tr['linked'], tr5['linked']))
        # the rule's own identities: every ring in one track, the degrees are the accepted rows
        assert int(tk['nrings'].sum()) == sum(t.size for t in tables)
        for t in range(KR.NSTEP - 1):
            r, ok = rows[t], tr['linked'][t]
            assert np.array_equal(ok, (r['a'] >= 0) & (r['b'] >= 0))                            # min_overlap 0: every pair of two rings
            assert np.array_equal(np.bincount(r['a'][ok], minlength=tables[t].size), tr['nnext'][t])
            assert np.array_equal(np.bincount(r['b'][ok], minlength=tables[t + 1].size), tr['nprev'][t + 1])
    assert merged and split and seam and single and born and weak
