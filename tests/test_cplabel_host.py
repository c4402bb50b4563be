"""The restatement of K20 (cplabel_ref.labels_of_masks, sets of nodes) and an independent one of the kernel's column scan
(cplabel_ref.scan_labels, chunks and carries included), on the CPU -- no GPU.  The records come from the restatements of K12, as in
test_cptree_host.py.  The scan must give the labels of the set rule on every hand-built plane of cptree_cases, on noise and on the
barotropic field; the three identities of the header hold; three broken scans each fail the case named for them."""
import numpy as np
import pytest

import cplabel_ref as LR
import cptree_cases as CS
import cptree_ref as TR
from test_cptree_host import records

# (name, plane, periodic): every plane of cptree_cases, each traced at level 0.5
PLANES = [('chain 13', CS.chain(13), 0), ('chain 83', CS.chain(83), 0), ('stacked siblings', CS.stacked_siblings(), 0),
          ('two blobs', CS.two_blobs(), 0), ('bands', CS.bands(), 1), ('seam', CS.seam(), 1), ('seam, plain', CS.seam(), 0),
          ('open above', CS.open_above(), 0), ('open beside NaN', CS.open_beside_nan(False), 0),
          ('open beside NaN, enclosed', CS.open_beside_nan(True), 0), ('checkerboard', CS.checkerboard(), 0),
          ('one node', CS.one_node(), 0), ('long walk, enclosed', CS.long_walk(True), 1), ('long walk', CS.long_walk(False), 1)]


def agree(rec, flip=0, rows=None):
    """the scan gives the labels of the set rule, and the header's three identities hold; -> (tables, labels) per range"""
    ny, nx = rec[4], rec[5]
    tables, masks = TR.piece_tree(*rec, flip=flip, return_masks=True)
    labels = [LR.labels_of_masks(ms, (ny, nx)) for ms in masks]
    for want, got in zip(labels, LR.scan_labels(*rec, flip=flip, rows=rows)):
        assert np.array_equal(want, got)
    for t, ms, lab in zip(tables, masks, labels):
        assert lab.dtype == np.int32 and lab.min() >= -1 and lab.max() < max(t.size, 1)
        assert not np.isin(lab, np.flatnonzero(~t['closed'])).any(), 'an open piece in the map'
        held = np.zeros((ny, nx), dtype=np.int64)
        for p in np.flatnonzero(t['closed']):
            assert (lab == p).sum() == t['n_net'][p]                          # the nodes labelled p are the net nodes of p
            under, q = np.zeros(t.size, dtype=bool), np.arange(t.size)
            for _ in range(int(t['depth'].max()) + 1):                        # p and its descendants: the rows whose chain of parents meets p
                under |= q == p
                q = np.where(q >= 0, t['parent'][np.maximum(q, 0)], -1)
            assert np.array_equal(np.isin(lab, np.flatnonzero(under)), ms[p])  # ... and with the descendants' they are I_p
            held += ms[p]
        assert np.array_equal(np.where(lab >= 0, t['depth'][np.maximum(lab, 0)] + 1, 0), held)   # depth[label] + 1 rings hold the node
    return tables, labels


@pytest.mark.parametrize('flip', [0, 1])
@pytest.mark.parametrize('name, q, periodic', PLANES, ids=[p[0] for p in PLANES])
def test_the_scan_is_the_set_rule_on_every_hand_built_plane(name, q, periodic, flip):
    (t,), (lab,) = agree(records(q, periodic), flip=flip)
    if t['closed'].any():
        assert (lab >= 0).any()
    if name.startswith('chain'):
        assert (lab == -1).sum() == 4 * (q.shape[0] - 1) and np.unique(lab).size == t.size + 1
    if name == 'seam, plain':
        assert (lab == -1).all()                                              # nothing but open pieces


def test_the_labels_of_the_stacked_siblings_written_out():
    q = CS.stacked_siblings()
    (t,), (lab,) = agree(records(q, False))
    block, upper, lower, island = (int(np.flatnonzero(t['n_in'] == n)[0]) for n in (98, 20, 9, 1))
    want = np.full(q.shape, -1)
    want[1:15, 1:8] = block
    want[3:8, 2:6] = upper
    want[5, 3] = island
    want[10:13, 3:6] = lower
    assert np.array_equal(lab, want)


@pytest.mark.parametrize('flip', [0, 1])
def test_the_labels_of_the_two_rings_that_go_round_written_out(flip):
    (t,), (lab,) = agree(records(CS.bands(), True), flip=flip)
    above, upper, between, lower, below = range(5)                          # first_edge order
    want = np.full((9, 8), -1)
    if not flip:                                                             # the upper ring holds rows 3 .. 8, the lower one rows 6 .. 8
        want[3:6], want[6:] = upper, lower
    else:                                                                    # the lower ring holds rows 0 .. 5, the upper one rows 0 .. 2
        want[0:3], want[3:6] = upper, lower
    want[1, 2], want[4, 4], want[7, 5] = above, between, below
    assert np.array_equal(lab, want)


@pytest.mark.parametrize('rows', [1, 2, 5, 600])
def test_any_chunk_length_gives_the_same_labels(rows):
    for q, periodic in ((CS.stacked_siblings(), 0), (CS.bands(), 1), (CS.open_beside_nan(True), 0), (CS.long_walk(True), 1)):
        for flip in (0, 1):
            agree(records(q, periodic), flip=flip, rows=rows)


def test_the_launch_regimes():
    assert LR.scan_geometry(2) == (16, 1) and LR.scan_geometry(16) == (16, 1) and LR.scan_geometry(17) == (16, 2)
    assert LR.scan_geometry(24) == (16, 2) and LR.scan_geometry(512) == (16, 32) and LR.scan_geometry(513) == (17, 31)
    assert LR.scan_geometry(600) == (19, 32) and LR.scan_geometry(1801) == (57, 32)


@pytest.mark.parametrize('periodic', [False, True], ids=['plain', 'ring'])
@pytest.mark.parametrize('nx', [63, 64, 65])
def test_the_scan_is_the_set_rule_on_smooth_noise_with_a_nan_block(nx, periodic):
    q = CS.smooth_noise(24, nx, nx)
    q[5:8, 7:9] = np.nan
    lv = np.linspace(-1.8, 1.8, 7)
    deep, opened = 0, False
    for flip in (0, 1):
        tables, labels = agree(records(q, periodic, lv), flip=flip)
        deep = max(deep, max(int(t['depth'].max()) for t in tables if t.size))
        opened |= any((~t['closed']).any() for t in tables)
        assert any((lab >= 0).any() and (lab == -1).any() for lab in labels)
    assert deep >= 1 and opened


def test_the_scan_is_the_set_rule_on_the_barotropic_field(baro):
    q = baro[0].astype(np.float64)
    lv = np.quantile(q, [0.1, 0.3, 0.5, 0.7, 0.9])
    deep = 0
    for periodic, flip in ((True, 0), (True, 1), (False, 0)):
        tables, labels = agree(records(q, periodic, lv), flip=flip)
        assert any((lab >= 0).any() and (lab == -1).any() for lab in labels)
        deep = max(deep, max(int(t['depth'].max()) for t in tables if t.size))
    assert deep >= 1


# ------------------------------------------------------------------ three broken scans, each caught by its case
def caught(rec, wrong, flip=0):
    _, masks = TR.piece_tree(*rec, flip=flip, return_masks=True)
    want = [LR.labels_of_masks(ms, (rec[4], rec[5])) for ms in masks]
    return any(not np.array_equal(a, b) for a, b in zip(want, LR.scan_labels(*rec, flip=flip, wrong=wrong)))


def test_a_scan_whose_leave_keeps_the_ring_is_caught_by_the_stacked_siblings():
    assert caught(records(CS.stacked_siblings(), False), 'leave keeps the ring')
    assert caught(records(CS.one_node(), False), 'leave keeps the ring')     # below the only ring the state must be -1 again


def test_a_scan_that_ignores_flip_is_caught_by_the_two_rings_that_go_round():
    assert caught(records(CS.bands(), True), 'flip ignored', flip=1)
    assert not caught(records(CS.bands(), True), 'flip ignored', flip=0)


def test_a_scan_that_takes_open_pieces_for_rings_is_caught():
    assert caught(records(CS.open_beside_nan(True), False), 'open pieces are rings')
    (t,), (lab,) = agree(records(CS.open_beside_nan(True), False))
    assert (~t['closed']).any() and lab[5, 5] == int(np.argmax(t['n_in']))   # below the open piece: still the block
