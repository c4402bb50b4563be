"""The restatements of K19, K21 and K22 (cptree_ref, cpprops_ref, cpoverlap_ref) on the calls of test_gpu_ring_sums.py, without a GPU:
with the windows of the bound rule handed in they are ring_sums_cases.model -- the kernels' chain of private words, wave sums, staged
words, K19's subtraction, K21's fold, carry and one rounding -- bit for bit on every call, and every step of that chain, broken alone
(ring_sums_cases.DEFECTS), is caught by some call: the GPU tests could fail.  The report is printed (pytest -s shows it)."""
import math

import numpy as np
import pytest

import cinside_ref as IR
import cinside_sums_cases as SC
import cpoverlap_ref as OR
import cpprops_ref as QR
import ring_sums_cases as RC

LISTS = tuple(SC.batches()) + ('floor', 'per slab', 'float32 integrand', 'overflow', 'no wrap')


@pytest.mark.parametrize('kernel', RC.KERNELS)
def test_the_restatement_is_the_model_and_every_defect_is_caught_and_every_list_catches_one(kernel):
    caught, lists, seen = RC.model_report(kernel)
    print('\n%s: %d calls' % (kernel, seen))
    for d, names in caught.items():
        print('  %-48s caught by %3d calls, e.g. %s' % (d, len(names), sorted(names)[:1]))
    for name, ds in lists.items():
        print('  list %-20s catches %s' % (name, sorted(ds)))
    want = [d for d in RC.DEFECTS if kernel in RC.ONLY.get(d, RC.KERNELS)]
    assert sorted(caught) == sorted(want) and len(want) == {'k19': 6, 'k21': 10, 'k22': 8}[kernel]
    assert [d for d, names in caught.items() if not names] == [], 'a defect no call catches'
    assert set(lists) == set(LISTS) | {'k19': {'fold'}, 'k21': {'fold', 'per field'}, 'k22': set()}[kernel]
    assert [name for name, ds in lists.items() if not ds] == [], 'a list that catches no defect'
    # the lists written for a defect do catch it
    assert 'rounds at the floor' in lists['bound outside'] and 'keeps a term under the window' in lists['bottom'] & lists['floor']
    assert 'one window for all slabs' in lists['per slab'] and 'a chunk one limb off at shift 17' in lists['shifts alone']
    assert 'the float32 integrand multiplied in float32' in lists['float32 integrand'] and 'a carry lost between two words' in lists['absorption']
    if kernel != 'k19':
        assert 'the wave sum in 32 bits' in lists['no wrap'] & lists['many equal']
    if kernel == 'k21':
        assert {'one window for all fields', 'the tops of fields 4 to 7 from fields 0 to 3'} <= lists['per field']
        assert 'gross folded from rounded doubles' in lists['fold']
    if kernel == 'k22':
        assert 'the bound over the kept nodes only' in lists['bound outside']


def test_every_restatement_without_tops_is_what_it_was_and_with_tops_cuts_at_the_floor():
    rng = np.random.default_rng(5)
    v = OR.scaled(rng, (40,))
    assert OR.exact(v) == math.fsum(v.tolist()) == OR.exact(v, 33) == QR.exact_sum(v) == QR.exact_sum(v, 33)
    b = 13 - 160
    straddling = np.array([math.ldexp(SC.ONE_UP, b + 20), SC.p2(b), math.ldexp(SC.ONE_UP, b - 53), 5e-324, 0.0, math.nan])
    assert OR.exact(straddling, 13) == QR.exact_sum(straddling, 13) == IR.window_sum(straddling, 13) == SC.p2(b + 20) + SC.p2(b)
    assert OR.exact(straddling[:5]) == math.fsum(straddling[:5].tolist()) != OR.exact(straddling, 13)
    assert math.isnan(OR.exact(np.array([1.0, math.inf]), 13)) and math.isnan(QR.exact_sum([1.0, -math.inf], 13))
    la, lb, w, f = OR.cases()['cancellation']
    tops = IR.window_tops(w, f[None], 1, *la.shape)[0]
    assert OR.same(OR.overlap_of_maps(la, lb, w, f), OR.overlap_of_maps(la, lb, w, f, tops=tops)), 'inside the window the two agree'


def test_the_planes_put_the_terms_where_the_tests_say():
    for pl in (RC.rings('chain', 17, 17), RC.rings('nest', 12, 70), RC.rings('nest', 70, 70), RC.rings('round', 33, 64),
               RC.rings('round', 33, 128), RC.rings('nest', 70, 128), RC.rings('round', 70, 128)):
        t = pl['table']
        assert t.size >= 3 and int(pl['inner'].sum()) == t['n_net'][pl['target']] >= 40 and t['nchild'][pl['target']] == 1
        assert not (pl['inner'] & pl['outside']).any() and pl['outside'].sum() > 12
        if pl['kind'] == 'round':                                            # whole waves of 64 columns end their first chunk in the target
            assert pl['nx'] % 64 == 0 and pl['inner'][2:16].all() and t['winding'][pl['target']] != 0
        else:                                                                # a plain plane: no wave of 64 threads lies in one ring
            assert not pl['inner'][:, [0, -1]].any() and t['parent'][pl['target']] >= 0
    assert RC.rings('chain', 17, 17)['table'].size == 8
    for shape in ((12, 70), (70, 12), (33, 128)):
        for where in ('omitted', 'other pair'):
            pl = RC.maps(*shape, where)
            pairs = set(zip(np.where(pl['la'] < 0, -1, pl['la']).ravel().tolist(), np.where(pl['lb'] < 0, -1, pl['lb']).ravel().tolist()))
            assert pairs == {(-1, -1), RC.PAIR, RC.ONE_SIDED, RC.OTHER}
            assert (pl['outside'] & pl['kept']).any() == (where == 'other pair') and not (pl['outside'] & pl['inner']).any()
    assert RC.maps(33, 128)['inner'][2:16].all()
    # a batch lands whole on the target, at every placement
    for kernel in RC.KERNELS:
        for how, c, cases, vname, which in RC.batch_calls(kernel, 'bottom'):
            for j, k in enumerate(which):
                got = sorted(t for t in RC.list_terms(c, j) if t != 0.0)
                assert got == sorted(cases[k]['terms']), c['what']
