"""The graphs of cptrack_geometry_cases.py on the CPU -- no GPU.  Each HAS what its tag says (links with a > b, the chosen roots, the hub's
degree, steps whose min and max lie on neither end of a track, 9 synchronous rounds, every link rejected for its own reason); the answers
written out there are cptrack_ref.tracks_of's; the kernels' rounds (cptrack_ref.rounds_of) reach the union-find's roots on every one of
them within nring + 1 rounds; the closed forms of the two large graphs equal tracks_of at 2^10 + 300 rings; and each rule of
cptrack_ref.BROKEN_GEOMETRY is caught by a named case."""
import os
import re

import numpy as np
import pytest

import cptrack_geometry_cases as GC
import cptrack_ref as KR

CASES = GC.cases()
I32 = np.iinfo(np.int32)


@pytest.fixture(scope='module')
def refs():
    return {name: GC.reference(c) for name, c in CASES.items()}              # computed once, shared, never changed


def of_group(group):
    return [name for name, c in CASES.items() if c['group'] == group]


def test_the_constants_are_the_kernels():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'xcontour_amd', 'csrc', 'xc_cptrack.hip')
    with open(path) as f:
        src = f.read()
    assert re.search(r'constexpr int RT_TPB = (\d+);', src).group(1) == str(GC.RT_TPB)
    assert re.search(r'constexpr int64_t RT_MAX_BLOCKS = 1 << (\d+);', src).group(1) == str(GC.RT_MAX_BLOCKS.bit_length() - 1)
    assert GC.STRIDE == 1 << 24


@pytest.mark.parametrize('name', list(CASES))
def test_the_written_answers_are_the_rules_and_the_rounds_reach_its_roots(refs, name):
    c, ref = CASES[name], refs[name]
    assert c['tag'] and c['group']
    for key, v in c['want'].items():
        if key == 'rows':
            assert ref['rows'].tolist() == v, name
        elif key == 'first_ring':
            assert ref['rows']['first_ring'].tolist() == v, name
        else:
            assert ref[key].tolist() == v, (name, key)
    root, rounds = KR.rounds_of(c['nring'], c['la'], c['lb'], ref['link_ok'])
    assert np.array_equal(root, ref['root']) and rounds <= c['nring'] + 1
    assert GC.rounds_fixed(c, ref) in (rounds, None) and (rounds >= 2 or GC.rounds_fixed(c, ref) is not None)
    if c['group'] in ('direction', 'hub'):                                   # any link order: the same words
        d, p = GC.shuffled(c)
        again = GC.reference(d)
        assert not (np.array_equal(d['la'], c['la']) and np.array_equal(d['lb'], c['lb']))
        assert all(np.array_equal(again[k], ref[k]) for k in ('root', 'track', 'nprev', 'nnext', 'rows'))
        assert np.array_equal(again['link_ok'], ref['link_ok'][p])


# ------------------------------------------------------------------ 1. steps
@pytest.mark.parametrize('name', of_group('steps'))
def test_unsorted_steps_put_min_and_max_on_neither_end_of_a_track(refs, name):
    c, ref = CASES[name], refs[name]
    rows, step = ref['rows'], c['step']
    assert (np.diff(step.astype(np.int64)) < 0).any()
    largest = np.zeros(rows.size, dtype=np.int64)
    np.maximum.at(largest, ref['track'], np.arange(c['nring']))
    assert (rows['first_step'] != step[rows['first_ring']]).any(), 'first_step is step[first_ring] on every track'
    assert (rows['last_step'] != step[largest]).any(), 'last_step is the step of the largest ring on every track'
    if 'int32' in name:
        for v in (I32.min, I32.max):
            at = np.flatnonzero(step == v)
            assert at.size >= 1 and (rows['nrings'][ref['track'][at]] >= 2).all()
        assert rows['first_step'].min() == I32.min and rows['last_step'].max() == I32.max
        assert (rows['last_step'] < 0).any() and (rows['first_step'] > 0).any()          # a wrong initial word of 0 shows in either
    if 'permuted' in name:
        base = KR.cases()[name.rsplit(',', 1)[0]]
        assert np.array_equal(np.sort(step), base['step']) and np.array_equal(c['la'], base['la'])


# ------------------------------------------------------------------ 2. direction
def test_the_direction_cases_have_the_links_their_tags_name(refs):
    share = lambda c: float((c['la'] > c['lb']).mean())
    c = CASES['chain of 5000, labels permuted']
    assert round(share(c), 3) == 0.505 and (refs['chain of 5000, labels permuted']['root'] == 0).all()
    assert KR.rounds_of(c['nring'], c['la'], c['lb'], np.ones(4999, dtype=bool))[1] == 9
    assert share(CASES['chain of 5000, descending']) == 1.0 and (refs['chain of 5000, descending']['root'] == 0).all()
    c = CASES['600 rings, self links only']
    assert np.array_equal(c['la'], c['lb']) and refs['600 rings, self links only']['rows'].size == 600
    c = CASES['diamond with self links']
    assert int((c['la'] == c['lb']).sum()) == 4 and int((c['la'] < c['lb']).sum()) == 4
    assert all(CASES[name]['mo'] == 0 and CASES[name]['size'] is None for name in of_group('direction'))


# ------------------------------------------------------------------ 3. hubs
@pytest.mark.parametrize('name', of_group('hub'))
def test_a_hub_has_every_link_and_its_track_one_split_or_one_merger(refs, name):
    c, ref = CASES[name], refs[name]
    at, side = (0 if 'hub 0' in name else GC.HUB_N - 1), name[-1]
    nlink = c['la'].size
    assert c['nring'] == GC.HUB_N and nlink == 69999 + 23333 and np.unique(np.stack([c['la'], c['lb']]), axis=1).shape[1] == 69999
    mine, theirs = ('nnext', 'nprev') if side == 'a' else ('nprev', 'nnext')
    assert (c['l' + side] == at).all() and ref[mine][at] == nlink and ref[theirs][at] == 0
    assert ref['rows'].size == 1 and (ref['root'] == 0).all()
    row = ref['rows'][0]
    assert row['nsplit' if side == 'a' else 'nmerge'] == 1 and row['nmerge' if side == 'a' else 'nsplit'] == 23333
    assert (row['first_ring'], row['first_step'], row['last_step'], row['nrings']) == (0, 0, 999, GC.HUB_N)


# ------------------------------------------------------------------ 4. ranks, 5. rejected links
def test_the_rank_cases_have_the_roots_they_are_named_after(refs):
    for n in GC.ISOLATED:
        c = CASES['%d isolated rings' % n]
        assert c['nring'] == n and c['la'].size == 0
    for name, chosen in GC.ROOT_SETS.items():
        c, ref = CASES['1024 rings, roots %s' % name], refs['1024 rings, roots %s' % name]
        assert c['nring'] == 1024 and np.unique(ref['root']).tolist() == sorted(set(chosen) | {0})
        assert c['la'].size == 1024 - len(set(chosen) | {0})
    blocks = np.unique(refs['1024 rings, roots block 3 alone']['rows']['first_ring'] // GC.RT_TPB).tolist()
    assert blocks == [0, 3]                                                   # blocks 1 and 2 count no root


def test_every_link_of_the_rejected_case_is_rejected_for_its_own_reason(refs):
    c, ref = CASES['300 rings, 400 links, all rejected'], refs['300 rings, 400 links, all rejected']
    assert not ref['link_ok'].any() and ref['rows'].size == 300
    why = [(c['la'] < 0), (c['lb'] < 0), (c['ln'] == 0), (c['la'] >= 0) & (c['lb'] >= 0) & (c['ln'] >= 1)]
    assert [int(w.sum()) for w in why] == [100] * 4 and (np.sum(why, axis=0) == 1).all()
    assert KR.accepted(c['size'], c['la'], c['lb'], c['ln'], 0.0).sum() == 100      # the last hundred fall to the threshold alone
    assert KR.rounds_of(300, c['la'], c['lb'], ref['link_ok'])[1] == 1


# ------------------------------------------------------------------ 7. the large graphs' closed forms
@pytest.mark.parametrize('build', [GC.second_trip, lambda n: GC.second_trip_chained(n, 1 << 10)], ids=['pairs', 'chained tail'])
def test_the_closed_forms_are_the_rules_at_a_small_size(build):
    nring = (1 << 10) + GC.TAIL
    g, closed = build(nring)
    assert g['nring'] == nring and g['la'].size == nring and g['size'] is None and g['mo'] == 0.0
    ref = GC.reference(g)
    assert KR.same(closed, ref) and closed['rows'].dtype == KR.ROW_DTYPE
    assert (g['step'] < 0).any() and (g['step'] > 0).any() and (np.diff(g['step'].astype(np.int64)) < 0).any()
    root, rounds = KR.rounds_of(nring, g['la'], g['lb'], ref['link_ok'])
    assert np.array_equal(root, closed['root']) and 2 <= rounds <= nring + 1
    if build is GC.second_trip:
        assert closed['rows'].size == nring // 2 and (closed['rows']['nsplit'] == 1).all() and (closed['rows']['nmerge'] == 1).all()
    else:
        first = 1 << 10
        assert closed['rows'].size == first // 2 + 1 and closed['rows'][-1]['nrings'] == GC.TAIL and (closed['root'][first:] == first).all()
        # only links from `first` on join the tail, and without the last of them no ring of it has a second link behind it
        head = GC.reference(dict(g, la=g['la'][:first], lb=g['lb'][:first], ln=g['ln'][:first]))
        assert (head['rows']['nrings'] == 2).all()
        poison = GC.tail_poison(nring, first)
        assert (GC.reference(poison)['root'][first:] == 0).all() and poison['la'].size == nring


def test_the_large_graphs_take_a_second_trip_of_300():
    assert GC.STRIDE + GC.TAIL > GC.RT_MAX_BLOCKS * GC.RT_TPB and (GC.STRIDE + GC.TAIL) % 2 == 0
    la, lb = GC.pair_links(GC.STRIDE + GC.TAIL)
    assert la.size == GC.STRIDE + GC.TAIL and lb.max() == GC.STRIDE + GC.TAIL - 1 and (np.bincount(la)[::2] == 2).all()


# ------------------------------------------------------------------ the broken rules
EXPECT = {'first_step from the root': 'five rings, steps out of order', 'last_step from the last ring': 'five rings, steps out of order',
          'nsplit counts links': 'hub 0 of 70 000 as a', 'max size in the threshold': 'a size of 0', 'n >= 0 accepted': 'a size of 0'}


@pytest.mark.parametrize('broken', [b for b in KR.BROKEN_GEOMETRY if b in EXPECT])
def test_every_broken_rule_is_caught_by_a_named_case(refs, broken):
    caught = [name for name, c in CASES.items()
              if not name.startswith('100 000') and not KR.same(GC.reference(c, broken=broken), refs[name])]
    assert EXPECT[broken] in caught, (broken, caught)
    old = KR.cases()
    missed = [name for name, c in old.items() if not name.startswith('100 000')
              and KR.same(KR.tracks_of(c['nring'], c['step'], c['size'], c['la'], c['lb'], c['ln'], c['mo'], broken=broken),
                          KR.tracks_of(c['nring'], c['step'], c['size'], c['la'], c['lb'], c['ln'], c['mo']))]
    print('%s: caught by %d new cases; %d of %d small cases of cptrack_ref.cases() do not tell' % (broken, len(caught), len(missed), len(old) - 1))


def test_the_refusals_are_refused_and_a_check_of_a_alone_misses_two_of_them():
    assert set(EXPECT) | {'only a checked against nring'} == set(KR.BROKEN_GEOMETRY)
    missed = []
    for name, (case, at, link) in GC.refusals().items():
        c = CASES[case]
        bad = GC.with_link(c, at, link)
        assert not KR.refused(c['nring'], c['la'], c['lb']) and KR.refused(c['nring'], bad['la'], bad['lb']), name
        assert int((bad['la'] != c['la']).sum() + (bad['lb'] != c['lb']).sum()) >= 1 and 0 <= at < c['la'].size
        if not KR.refused(c['nring'], bad['la'], bad['lb'], broken='only a checked against nring'):
            missed.append(name)
    assert 'a negative a does not shield b == nring' in missed and 'a bad b in the last link of a launch of many blocks' in missed
    case, at, _ = GC.refusals()['a bad b in the last link of a launch of many blocks']
    assert at == CASES[case]['la'].size - 1 and at // GC.RT_TPB >= 300         # the last thread of a launch of hundreds of blocks
