"""The restatement of K18 (cpinside_ref.piece_interiors) and the kernel's mapping (cpinside_ref.mapping) on the CPU -- no GPU.  The
records come from the restatements of K12 (contour_join_ref, contour_join_periodic_ref), as in test_cinside_host.py.  First the
restatement on hand-built planes whose answers are written out; then the mapping -- orientation from the ids, one sign per ring,
alternation down a column -- against the parity rule on noise with NaN blocks and on the barotropic field; last, three broken
mappings that each fail a case."""
import numpy as np
import pytest

import contour_join_periodic_ref as JP
import contour_join_ref as JR
import cpinside_ref as PR


def records(q, periodic, levels):
    q = np.asarray(q, dtype=np.float64)
    rec = (JP if periodic else JR).stack_records(q[None], np.asarray(levels, dtype=np.float64))
    return rec + q.shape + (1 if periodic else 0,)


def agree(rec, flip=0):
    """the mapping gives the masks of the parity rule; -> (tables, masks) of the rule"""
    tables, masks = PR.piece_interiors(*rec, flip=flip, return_masks=True)
    assert PR.same_masks(PR.mapping(*rec, flip=flip), masks)
    return tables, masks


# ------------------------------------------------------------------ the restatement on hand-built planes
@pytest.mark.parametrize('periodic', [False, True], ids=['plain', 'ring'])
def test_a_one_node_blob(periodic):
    q = np.zeros((5, 6))
    q[2, 3] = 1.0
    (t,), (m,) = agree(records(q, periodic, (0.5,)))
    assert t.size == 1 and t['nseg'][0] == 4 and t['closed'][0] and t['winding'][0] == 0 and t['n_in'][0] == 1
    assert m[0][2, 3] and m[0].sum() == 1 and t['sum_w'][0] == 1.0 and np.isnan(t['sum_wf'][0])
    # a hole instead of a blob: the ring runs the other way round, the interior is the same node
    (t2,), (m2,) = agree(records(1.0 - q, periodic, (0.5,)))
    assert t2['n_in'].tolist() == [1] and np.array_equal(m2[0], m[0])


def test_a_ring_round_a_2_x_3_block_with_weights():
    q = np.zeros((6, 7))
    q[2:4, 1:4] = 1.0
    w = np.arange(42, dtype=np.float64).reshape(6, 7)
    f = np.full((1, 6, 7), 0.5)
    (t,) = PR.piece_interiors(*records(q, False, (0.5,)), w=w, f=f)
    assert t['nseg'].tolist() == [10] and t['n_in'].tolist() == [6]
    assert t['sum_w'][0] == w[2:4, 1:4].sum() and t['sum_wf'][0] == 0.5 * w[2:4, 1:4].sum()
    agree(records(q, False, (0.5,)))


def nested():
    """a 7 x 7 block of ones with a 3 x 3 hole of zeros and a single one in the middle of the hole: three rings, one in the other"""
    q = np.zeros((11, 12))
    q[2:9, 2:9] = 1.0
    q[4:7, 4:7] = 0.0
    q[5, 5] = 1.0
    return q


@pytest.mark.parametrize('periodic', [False, True], ids=['plain', 'ring'])
def test_a_ring_nested_in_a_ring_the_outer_counts_the_inner_nodes(periodic):
    (t,), _ = agree(records(nested(), periodic, (0.5,)))
    assert sorted(t['n_in'].tolist()) == [1, 9, 49] and t['closed'].all() and (t['winding'] == 0).all()
    assert t['n_in'][np.argmin(t['first_edge'])] == 49                        # the outer ring touches the smallest edge id


def test_two_blobs_in_one_column_each_gets_its_own_nodes():
    q = np.zeros((12, 6))
    q[2:4, 2] = 1.0
    q[6:11, 2:4] = 1.0
    (t,), (m,) = agree(records(q, False, (0.5,)))
    assert t['n_in'].tolist() == [2, 10]
    assert m[0][2:4, 2].all() and m[0].sum() == 2 and m[1][6:11, 2:4].all() and m[1].sum() == 10


def s_fold(ny=12, nx=9):
    """a circumpolar contour with an S-fold: rows >= 6 are above the level, but for a tongue of high values that reaches up and then
    sideways over low ones in columns 3 to 5"""
    q = np.zeros((ny, nx))
    q[6:] = 1.0
    q[2:6, 3] = 1.0
    q[2, 3:6] = 1.0
    return q


@pytest.mark.parametrize('flip', [0, 1])
def test_a_circumpolar_ring_with_an_s_fold(flip):
    q = s_fold()
    (t,), (m,) = agree(records(q, True, (0.5,)), flip=flip)
    assert t.size == 1 and t['closed'][0] and abs(t['winding'][0]) == 1
    assert np.array_equal(m[0], (q > 0.5) ^ bool(flip))
    assert t['n_in'][0] == (int((q > 0.5).sum()) if not flip else int((q <= 0.5).sum()))
    # column 5 meets the ring three times
    assert PR.IR.crossing_flags(*records(q, True, (0.5,)), 'all')[0][:, 5].sum() == 3
    # a ring of winding 0 beside it is not flipped
    q[9, 1] = 0.0
    (t,), _ = agree(records(q, True, (0.5,)), flip=flip)
    assert sorted(t['n_in'].tolist())[0] == 1 and sorted(np.abs(t['winding']).tolist()) == [0, 1]


def test_an_open_chain_bounds_nothing():
    q = np.zeros((6, 7))
    q[3:] = 1.0
    (t,), (m,) = agree(records(q, False, (0.5,)))
    assert t.size == 1 and not t['closed'][0] and t['n_in'][0] == -1 and np.isnan(t['sum_w'][0]) and np.isnan(t['sum_wf'][0]) and m[0] is None


@pytest.mark.parametrize('periodic', [False, True], ids=['plain', 'ring'])
def test_a_level_exactly_on_node_values(periodic):
    q = np.random.default_rng(11).integers(-2, 3, (14, 13)).astype(np.float64)
    rec = records(q, periodic, (-1.0, 0.0, 1.0))
    tables, masks = agree(rec)
    assert sum(int(t['closed'].sum()) for t in tables) > 6
    # a ring of winding 0 encloses nodes of one kind along its inner side: the interiors of all rings of a level, nested ones taken
    # once more each, rebuild the threshold mask away from the open pieces
    for t in tables:
        assert (t['n_in'][t['closed']] >= 1).all() and (t['n_in'][~t['closed']] == -1).all()


# ------------------------------------------------------------------ the mapping against the parity rule
def blocked_noise(ny, nx, seed):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((ny, nx)) + np.linspace(-1.5, 1.5, ny)[:, None]
    q[ny // 3:ny // 3 + 2, nx // 4:nx // 4 + 3] = np.nan
    q[ny - 4, nx - 1] = np.nan
    q[0, 0] = np.nan
    q[rng.integers(0, ny, 6), rng.integers(0, nx, 6)] = np.nan
    return q


@pytest.mark.parametrize('periodic', [False, True], ids=['plain', 'ring'])
@pytest.mark.parametrize('nx', [63, 64, 65])
def test_the_mapping_is_the_parity_rule_on_nan_blocked_noise(nx, periodic):
    q = blocked_noise(21, nx, 100 + nx)
    lv = np.array([-1.0, 0.0, q[5, 5], 0.9])
    lv = np.sort(lv[np.isfinite(lv)])
    for flip in (0, 1):
        tables, _ = agree(records(q, periodic, lv), flip=flip)
    assert sum(int(t['closed'].sum()) for t in tables) > 30 and sum(int((~t['closed']).sum()) for t in tables) > 3


def test_the_mapping_is_the_parity_rule_on_the_barotropic_field(baro):
    q = np.asarray(baro[0], dtype=np.float64)
    lv = np.quantile(q, [0.35, 0.8])
    for flip in (0, 1):
        tables, _ = agree(records(q, True, lv), flip=flip)
    assert all((t['winding'] != 0).any() for t in tables)
    assert sum(int((t['closed'] & (t['winding'] == 0)).sum()) for t in tables) >= 1


# ------------------------------------------------------------------ three broken mappings, each caught
def caught(rec, wrong, flip=0):
    _, masks = PR.piece_interiors(*rec, flip=flip, return_masks=True)
    try:
        return not PR.same_masks(PR.mapping(*rec, flip=flip, wrong=wrong), masks)
    except (AssertionError, IndexError):                                     # two walks met, or one left the plane
        return True


def test_a_sign_that_is_not_per_piece_is_caught():
    q = np.zeros((5, 6))
    q[2, 3] = 1.0
    assert caught(records(q, False, (0.5,)), 'sign not per piece') != caught(records(1.0 - q, False, (0.5,)), 'sign not per piece')


def test_an_exit_row_that_is_included_is_caught():
    q = np.zeros((5, 6))
    q[2, 3] = 1.0
    assert caught(records(q, False, (0.5,)), 'exit row included')


def test_nested_nodes_that_are_subtracted_are_caught():
    assert caught(records(nested(), False, (0.5,)), 'nested nodes subtracted')
    q = np.zeros((5, 6))
    q[2, 3] = 1.0
    assert not caught(records(q, False, (0.5,)), 'nested nodes subtracted')   # a single blob cannot tell


# ------------------------------------------------------------------ the windows of the sums (K17's rule, cinside_ref.window_tops)
import cinside_sums_cases as SC
import cpiece_records_ref as RR
from test_gpu_cpinside_records import noise, scaled


@pytest.mark.parametrize('periodic', [False, True], ids=['plain', 'ring'])
def test_on_the_scaled_inputs_of_the_records_suite_the_window_changes_nothing(periodic):
    """exponents in [-20, 20]: every term lies wholly inside its window, so the sums of the header's rule ARE plain math.fsum, bit for
    bit -- what test_gpu_cpinside_records.py asserted before the reference stated the window, it asserts still"""
    ny, nx = 33, 40
    q = noise(ny, nx, 2, 90 + ny + nx)
    lv = np.sort(np.array([-0.7, q[1, 3, 3], 0.8]))
    rec = (JP if periodic else JR).stack_records(q, lv) + (ny, nx, int(periodic))
    rng = np.random.default_rng(92 + nx)
    w2, w3 = scaled(rng, (ny, nx)), scaled(rng, (2, ny, nx))
    f32, f64 = scaled(rng, (2, ny, nx), np.float32), scaled(rng, (2, ny, nx))
    w2[5, 5], f64[1, 7, 7] = np.nan, np.nan
    for w, f in ((w2, f64), (w3, f32), (None, None), (None, f64)):
        tables, masks, tops = PR.piece_interiors(*rec, flip=1, ncont=3, w=w, f=f, return_masks=True, return_tops=True)
        assert len(tops) == 2 and all(-8 <= tw <= 33 and (tf is None or -28 <= tf <= 53) for tw, tf in tops)
        nclosed = 0
        for r, (t, ms) in enumerate(zip(tables, masks)):
            ws, wf = PR.IR.slab_planes(w, f, r // 3, ny, nx)
            for row, m in zip(t, ms):
                if m is None:
                    continue
                nclosed += 1
                assert SC.same(row['sum_w'], PR.IR.nan_skipping_sum(ws[m]))
                assert np.isnan(row['sum_wf']) if f is None else SC.same(row['sum_wf'], PR.IR.nan_skipping_sum(wf[m]))
        assert nclosed > 20


@pytest.mark.parametrize('kind', [k for k in SC.KINDS if k.startswith('k18')])
def test_the_limb_model_on_k18s_windows_every_defect_caught_by_the_list_written_for_it(kind):
    """block ring (walks down), comb ring without flip (down) and with flip (up): the same term lists, the same windows"""
    caught, seen = SC.limb_model_report(kind)
    assert seen > 1000
    for d in RR.DEFECTS:
        assert SC.CATCHES[d] <= caught[d], (d, sorted(SC.CATCHES[d] - caught[d]))
