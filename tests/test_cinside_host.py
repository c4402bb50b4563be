"""The restatement of K17 (cinside_ref) on the CPU -- no GPU.  The records come from the restatements of K12 (contour_join_ref,
contour_join_periodic_ref), as in test_coverturn_host.py.  What is shown: on a NaN-free field 'all' reproduces the threshold mask
relative to row 0 exactly, levels on node values included; the flags of a column add up to K16's ncross; the selection matters (a
cut-off blob and a hole); beside NaN cells the mask follows the records, not the threshold."""
import numpy as np
import pytest

import cinside_ref as IR
import contour_join_periodic_ref as JP
import contour_join_ref as JR
import coverturn_ref as OR


def records(q, periodic, levels):
    rec = (JP if periodic else JR).stack_records(np.asarray(q, dtype=np.float64)[None], np.asarray(levels, dtype=np.float64))
    return rec + q.shape + (1 if periodic else 0,)


def noise(ny, nx, seed):
    """integers in [-3, 3]: many nodes ON the integer levels"""
    return np.random.default_rng(seed).integers(-3, 4, (ny, nx)).astype(np.float64)


LEVELS = np.array([-2.5, -1.0, 0.0, 0.25, 1.0, 2.0, 2.75])


@pytest.mark.parametrize('periodic', [False, True], ids=['plain', 'ring'])
@pytest.mark.parametrize('shape', [(2, 2), (3, 5), (9, 12), (17, 6)])
def test_all_on_a_nan_free_field_is_the_threshold_mask_relative_to_row_0(shape, periodic):
    for seed in (1, 2):
        q = noise(*shape, seed) if seed == 1 else np.random.default_rng(seed).standard_normal(shape)
        lv = LEVELS if seed == 1 else np.sort(np.concatenate([LEVELS / 2.0, q.ravel()[:3]]))      # levels equal to node values
        assert np.isin(lv, q).any()
        out = IR.interior(*records(q, periodic, lv), 'all')
        above = q[None] > lv[:, None, None]
        assert np.array_equal(out['mask'].astype(bool), above ^ above[:, :1])
        flipped = IR.interior(*records(q, periodic, lv), 'all', flip=1)
        assert np.array_equal(flipped['mask'], 1 - out['mask']) and np.array_equal(flipped['n_in'] + out['n_in'], np.full(lv.size, q.size))
        # weight 1: the sum is the count; a weight plane: fsum over the mask
        assert np.array_equal(out['sum_w'], out['n_in'].astype(np.float64)) and out['sum_wf'] is None
        w = np.random.default_rng(3).random(shape)
        got = IR.interior(*records(q, periodic, lv), 'all', w=w, f=q[None])
        assert got['sum_w'].tolist() == [IR.nan_skipping_sum(w[m]) for m in out['mask'].astype(bool)]
        assert got['sum_wf'].tolist() == [IR.nan_skipping_sum(w[m] * q[m]) for m in out['mask'].astype(bool)]


@pytest.mark.parametrize('periodic,select', [(False, 'all'), (True, 'all'), (True, 'circumpolar'), (True, 'main')])
def test_the_flags_of_a_column_add_up_to_the_crossings_of_k16(periodic, select):
    q = np.random.default_rng(4).standard_normal((12, 15))
    q[6:] += 2.5                                                              # a step the middle levels follow round the ring
    lv = np.array([-1.0, 0.3, 1.2, 1.5, 2.0, 9.0])
    rec = records(q, periodic, lv)
    X = IR.crossing_flags(*rec, select)
    ref = OR.overturning(*rec, select)
    assert np.array_equal(X.sum(axis=1), ref['ncross'])
    assert X.sum() > 0 and not X[-1].any()
    if select == 'main':
        assert (ref['main_first_edge'][1:5] >= 0).any() and (X.sum(axis=(1, 2)) < IR.crossing_flags(*rec, 'all').sum(axis=(1, 2))).any()


NY, NX = 10, 12


def shed():
    """a zonal gradient (q = the row), one detached blob above the level 4.5 at node (2, 5), one hole below it at node (7, 8)"""
    q = np.repeat(np.arange(NY, dtype=np.float64)[:, None], NX, axis=1)
    q[2, 5] = 9.0
    q[7, 8] = 0.0
    return q


def test_main_is_the_cap_alone_and_all_adds_the_blob_and_removes_the_hole():
    q = shed()
    rec = records(q, True, (4.5,))
    cap = np.zeros((NY, NX), dtype=np.uint8)
    cap[5:] = 1
    main = IR.interior(*rec, 'main')
    assert np.array_equal(main['mask'][0], cap) and main['n_in'].tolist() == [5 * NX]
    every = IR.interior(*rec, 'all')
    expect = cap.copy()
    expect[2, 5], expect[7, 8] = 1, 0
    assert np.array_equal(every['mask'][0], expect) and np.array_equal(expect.astype(bool), q > 4.5)
    assert every['n_in'].tolist() == [5 * NX]                                # one node shed, one node lost: the counts agree, the masks do not
    circ = IR.interior(*rec, 'circumpolar')
    assert np.array_equal(circ['mask'], main['mask'])
    # the area shed and the area of the hole, with a weight that tells them apart
    w = np.ones((NY, NX))
    w[2, 5], w[7, 8] = 0.25, 4.0
    assert IR.interior(*rec, 'main', w=w)['sum_w'].tolist() == [5 * NX + 3.0]
    assert IR.interior(*rec, 'all', w=w)['sum_w'].tolist() == [5 * NX - 1 + 0.25]
    # the other side
    low = IR.interior(*rec, 'main', flip=1)
    assert np.array_equal(low['mask'][0], 1 - cap) and low['n_in'].tolist() == [5 * NX]
    with pytest.raises(ValueError):
        IR.interior(*records(q, False, (4.5,)), 'main')


@pytest.mark.parametrize('periodic', [False, True], ids=['plain', 'ring'])
def test_beside_nan_cells_the_mask_follows_the_records_not_the_threshold(periodic):
    """a step between rows 3 and 4 with a NaN at node (4, 5): both vertical edges of column 5 that could carry the crossing touch the
    NaN node, no NaN-free cell sees one there, and the whole column stays on row 0's side.  The columns beside it keep their
    crossing: the cells (3, 3) and (3, 6) see it."""
    q = np.zeros((8, 12))
    q[4:] = 1.0
    q[4, 5] = np.nan
    out = IR.interior(*records(q, periodic, (0.5,)), 'all')
    expect = np.zeros((8, 12), dtype=np.uint8)
    expect[4:] = 1
    expect[:, 5] = 0
    assert np.array_equal(out['mask'][0], expect)
    with np.errstate(invalid='ignore'):
        threshold = q > 0.5
    differ = np.argwhere(out['mask'][0].astype(bool) != threshold)
    assert differ.tolist() == [[5, 5], [6, 5], [7, 5]]                       # under the NaN node; the node itself is outside under both rules
    # sums skip a NaN term and an infinite one poisons its range alone
    w = np.ones((8, 12))
    w[6, 2] = np.nan
    w[0, 0] = np.inf
    both = IR.interior(*records(q, periodic, (0.5, 5.0)), 'all', w=w)
    assert both['sum_w'][0] == out['n_in'][0] - 1 and both['sum_w'][1] == 0.0
    flipped = IR.interior(*records(q, periodic, (0.5, 5.0)), 'all', flip=1, w=w)
    assert np.isnan(flipped['sum_w']).all()
