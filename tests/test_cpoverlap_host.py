"""K22's two restatements agree (no GPU): cpoverlap_ref.scan_of_maps -- the kernel's run walk per column chunk -- gives the rows of
cpoverlap_ref.overlap_of_maps -- np.unique over the pairs, math.fsum of the terms -- on every case of the GPU tests, at chunk lengths 1,
2, 5 and 600.  And the cases can fail: each of four deliberately broken walks is caught by at least one of them."""
import numpy as np
import pytest

import cpoverlap_ref as OR

CASES = OR.cases()


@pytest.mark.parametrize('name', list(CASES))
def test_the_run_walk_gives_the_rows_of_the_set_rule_at_every_chunk_length(name):
    la, lb, w, f = CASES[name]
    ref = OR.overlap_of_maps(la, lb, w, f)
    for chunk in (1, 2, 5, 600):
        assert OR.same(OR.scan_of_maps(la, lb, w, f, chunk=chunk), ref), chunk
    # the marginals: the rows of a label partition its nodes
    for key, m in (('a', la), ('b', lb)):
        for lab in np.unique(m[m >= 0]).tolist():
            assert ref['n'][ref[key] == lab].sum() == (m == lab).sum()
    # the runs bound the distinct pairs
    for chunk in (1, 16, 600):
        assert OR.count_runs(la, lb, chunk) >= ref.size


def test_what_the_cases_hold():
    sizes = {k: OR.overlap_of_maps(*v).size for k, v in CASES.items()}
    assert sizes['both all -1'] == 0 and sizes['stripes'] == 4225 and sizes['one pair but one node'] == 2
    d = OR.overlap_of_maps(*CASES['identical maps'])
    assert d.size > 3 and (d['a'] == d['b']).all()
    big = OR.overlap_of_maps(*CASES['labels 2^31 - 1 and 0'])
    assert (big['a'] == 2 ** 31 - 1).any() and (big['a'] == 0).any()
    neg = OR.overlap_of_maps(*CASES['labels -7 and INT32_MIN'])
    assert neg['a'].min() == -1 and neg['b'].min() == -1 and ((neg['a'] == -1) & (neg['b'] == 4)).any()
    assert OR.count_runs(*CASES['stripes'][:2], 16) == 4225


@pytest.mark.parametrize('broken', OR.BROKEN)
def test_every_broken_walk_is_caught_by_a_case(broken):
    caught = [name for name, (la, lb, w, f) in CASES.items()
              if not OR.same(OR.scan_of_maps(la, lb, w, f, chunk=16, broken=broken), OR.overlap_of_maps(la, lb, w, f))]
    assert caught, 'no case catches %r' % broken


def test_the_sums_follow_k17s_rules():
    la, lb = np.zeros((4, 4), dtype=np.int32), np.zeros((4, 4), dtype=np.int32)
    lb[2:] = 1
    w, f = np.ones((4, 4)), np.ones((4, 4))
    w[0, 0], f[3, 3] = np.nan, np.inf
    rows = OR.overlap_of_maps(la, lb, w, f)
    assert rows['n'].tolist() == [8, 8] and rows['sum_w'].tolist() == [7.0, 8.0]
    assert rows['sum_wf'][0] == 7.0 and np.isnan(rows['sum_wf'][1])
