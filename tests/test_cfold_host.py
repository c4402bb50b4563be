"""The restatement of K24 (cfold_ref) on the CPU -- no GPU.  The records come from the restatements of K12 (contour_join_ref,
contour_join_periodic_ref) on the hand-built planes of cfold_ref.cases(): q = far ? 1 : 0 with level 0.5, so the crossings are exactly
the mask's transitions down a column.  What is shown: the events of every plane are the ones the plane was drawn with; every
deliberately broken rule of cfold_ref.WRONG changes at least one case; the sums are plain math.fsum on these weights; and the package
declares the entry and the method (which fails before K24)."""
import math
import os

import numpy as np
import pytest

import cfold_ref as FR
import cinside_ref as IR
import contour_join_periodic_ref as JP
import contour_join_ref as JR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = {k: v for k, v in FR.cases().items() if v[0].shape[1] <= 70}          # (the widest planes run on the GPU)


def records(m, periodic):
    q = FR.field(m)
    return (JP if periodic else JR).stack_records(q[None], FR.LEVEL)


def weights(shape, seed=5):
    rng = np.random.default_rng(seed)
    w = np.ldexp(rng.uniform(1.0, 2.0, shape), rng.integers(-20, 20, shape))
    f = (np.ldexp(rng.uniform(1.0, 2.0, shape), rng.integers(-20, 20, shape)) * rng.choice([-1.0, 1.0], shape))[None]
    return w, f


def ref(name, wrong=None, weighted=True):
    m, periodic, select, gap = SMALL[name]
    w, f = weights(m.shape) if weighted else (None, None)
    return FR.folds(*records(m, periodic), *m.shape, periodic, select, gap=gap, w=w, f=f, wrong=wrong)


def test_the_crossings_of_a_mask_plane_are_its_transitions():
    for name, (m, periodic, select, gap) in SMALL.items():
        if select != 0:
            continue
        X = IR.crossing_flags(*records(m, periodic), *m.shape, periodic, select)
        assert np.array_equal(X[0], (m[1:] != m[:-1]).astype(np.uint8)), name


EXPECT = {                       # name -> (c_west, c_east, ncol, ncross_max, nodes [under, over] per event)
    'no fold': ([], [], [], [], []),
    'hook of 3': ([3], [4], [2], [3], [[4, 4]]),
    'hook of 5': ([3], [4], [2], [5], [[6, 6]]),
    'two hooks, gap 0': ([2, 5], [3, 6], [2, 2], [3, 3], [[4, 4], [4, 6]]),
    'two hooks, gap 1': ([2], [6], [4], [3], [[8, 10]]),
    'two hooks, gap 2': ([2], [6], [4], [3], [[8, 10]]),
    'seam hook, ring': ([7], [0], [2], [3], [[4, 4]]),
    'seam hook, plain': ([0, 7], [0, 7], [1, 1], [3, 3], [[2, 2], [2, 2]]),
    'every column folded': ([0], [7], [8], [3], [[16, 16]]),
    'every column folded, gap 3': ([0], [7], [8], [3], [[16, 16]]),
    'blob, all': ([3], [4], [2], [3], [[4, 4]]),
    'blob, main': ([], [], [], [], []),
    'two crossings': ([], [], [], [], []),
    'nx 33': ([31], [32], [2], [3], [[4, 4]]),
    'nx 65': ([30, 63], [33, 64], [4, 2], [3, 3], [[8, 12], [4, 4]]),
}


@pytest.mark.parametrize('name', sorted(EXPECT))
def test_the_events_of_every_hand_built_plane_are_the_ones_it_was_drawn_with(name):
    out = ref(name)
    cw, ce, ncol, nmax, nodes = EXPECT[name]
    assert out['event_count'].tolist() == [len(cw)]
    assert (out['c_west'].tolist(), out['c_east'].tolist(), out['ncol'].tolist(), out['ncross_max'].tolist()) == (cw, ce, ncol, nmax)
    assert out['nodes'].tolist() == nodes
    m = SMALL[name][0]
    nx = m.shape[1]
    # the labels: the folded columns of event j going east from c_west, nothing else
    want = np.full(nx, -1)
    for j, (a, b) in enumerate(zip(cw, ce)):
        for c in [(a + d) % nx for d in range((b - a) % nx + 1)]:
            if out['ncross'][0, c] >= 3:
                want[c] = j
    assert np.array_equal(out['col_event'][0], want)
    assert np.array_equal(np.isnan(out['row_lo']), out['ncross'] == 0)


def test_the_tongues_of_a_hook_and_their_sums_are_plain_fsum():
    """hook of 3 over columns 3, 4 of a 9 x 8 plane: far rows 2, 3 (the tongue), near rows 4, 5, far from row 6 on.  Crossings on the
    edges under rows 1, 3, 5: lo = 1, hi = 5.  Fold nodes rows 2 .. 5: rows 2, 3 lie beyond the lowest crossing (under), rows 4, 5 are
    row 0's air above them (over)."""
    m = SMALL['hook of 3'][0]
    w, f = weights(m.shape)
    out = ref('hook of 3')
    for t, rows in ((0, (2, 3)), (1, (4, 5))):
        nodes = [(r, c) for c in (3, 4) for r in rows]
        assert FR.same_bits(out['area'][0, t], math.fsum(w[n] for n in nodes))
        assert FR.same_bits(out['mx'][0, t], math.fsum(w[r, c] * (c - 3) for r, c in nodes))
        assert FR.same_bits(out['my'][0, t], math.fsum(w[r, c] * r for r, c in nodes))
        assert FR.same_bits(out['integral'][0, t], math.fsum(w[n] * f[0][n] for n in nodes))
    assert out['ev_row_lo'].tolist() == [1.5] and out['ev_row_hi'].tolist() == [5.5]
    bare = ref('hook of 3', weighted=False)
    assert bare['integral'] is None and np.array_equal(bare['area'], bare['nodes'].astype(np.float64))
    # the windows on these weights cut nothing
    assert all(-8 <= t[0] <= 33 and t[0] < t[1] <= t[0] + 4 for t in out['tops'])


@pytest.mark.parametrize('wrong', FR.WRONG)
def test_every_broken_rule_changes_at_least_one_case(wrong):
    caught = [name for name in SMALL if FR.differences(ref(name, wrong), ref(name)) != []]
    assert caught, wrong
    want = {'n >= 2': 'two crossings', 'no seam join': 'seam hook, ring', 'gap ignored': 'two hooks, gap 1',
            'bridged columns labelled': 'two hooks, gap 1', 'tongue from P alone': 'hook of 3', 'dx without mod': 'seam hook, ring',
            'hi excluded': 'hook of 5'}[wrong]
    assert want in caught, (wrong, caught)


def test_gap_must_lie_below_nx_and_select_needs_a_ring():
    m = SMALL['hook of 3'][0]
    with pytest.raises(AssertionError):
        FR.folds(*records(m, 1), *m.shape, 1, 2, gap=8)
    with pytest.raises(ValueError):
        FR.folds(*records(m, 0), *m.shape, 0, 2)


def test_the_package_declares_the_entry_and_the_method():
    from xcontour_amd import core
    assert callable(getattr(core.Contour2D, 'cal_contour_folds', None))
    with open(os.path.join(ROOT, 'include', 'xcontour_hip.h')) as fh:
        header = fh.read()
    assert 'int xc_contour_folds_dev(' in header and 'int xc_last_cfold_profile(' in header
