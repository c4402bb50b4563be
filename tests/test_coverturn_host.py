"""The restatement of K16 (coverturn_ref.overturning) on cases counted by hand -- no GPU.  Every case is also run through the broken
variants of the rule (coverturn_ref.WRONG), and each of them is shown to fail a case: the GPU tests compare against a restatement
that can tell.  The records come from the restatements of K12 (contour_join_ref, contour_join_periodic_ref) on 0 / 1 fields traced
at 0.5, so every crossing row is k + 0.5 exactly."""
import numpy as np
import pytest

import contour_join_periodic_ref as JP
import contour_join_ref as JR
import coverturn_ref as OR

NY, NX = 8, 12


def records(q, periodic, levels=(0.5,)):
    rec = (JP if periodic else JR).stack_records(np.asarray(q, dtype=np.float64)[None], np.asarray(levels, dtype=np.float64))
    return rec + q.shape + (1 if periodic else 0,)


def run(q, periodic, select, wrong=None, levels=(0.5,)):
    return OR.overturning(*records(q, periodic, levels), select, wrong=wrong)


def step(row):
    """low (0) above node row `row`, high (1) from it on: one zonal contour at row - 0.5"""
    q = np.zeros((NY, NX))
    q[row:] = 1.0
    return q


def fold():
    """an S-shaped fold of the one circumpolar contour: a high tongue at rows 2-3 over columns 4-7, hanging on column 7, above a low
    pocket at rows 4-5 over columns 3-6, open towards column 3"""
    q = step(4)
    q[2:4, 4:8] = 1.0
    q[4:6, 3:7] = 0.0
    return q


def blob():
    """the zonal contour at 3.5 and, cut off from it, one high node at (1, 5)"""
    q = step(4)
    q[1, 5] = 1.0
    return q


def band(bump):
    """high on rows 3-4 only: two zonal rings, at 2.5 and at 4.5, of opposite winding; bump: node (5, 6) high too, which gives the
    lower ring two more segments"""
    q = np.zeros((NY, NX))
    q[3:5] = 1.0
    if bump:
        q[5, 6] = 1.0
    return q


def expect(out, ncross, lo, hi):
    assert out['ncross'].tolist() == [list(ncross)]
    assert OR.same_bits(out['row_lo'], [lo]) and OR.same_bits(out['row_hi'], [hi])


def test_zonal_contours_on_a_ring_cross_every_meridian_once():
    q = np.repeat(np.arange(NY, dtype=np.float64)[:, None], NX, axis=1)
    lv = (1.5, 2.25, 6.5)
    for select in ('all', 'circumpolar', 'main'):
        out = run(q, True, select, levels=lv)
        assert (out['ncross'] == 1).all() and OR.same_bits(out['row_lo'], out['row_hi'])
        assert OR.same_bits(out['row_lo'], np.repeat(np.array(lv)[:, None], NX, axis=1))
        assert (np.abs(out['main_winding']) == 1).all() and (out['main_nseg'] == NX).all() and (out['nsel'] == 1).all()
        # the ring's smallest id: the vertical edge V(floor(level), 0)
        assert out['main_first_edge'].tolist() == [2 * (int(v) * NX) + 1 for v in lv]
    down = run(-q, True, 'main', levels=(-1.5,))
    assert down['main_winding'][0] == -run(q, True, 'main', levels=(1.5,))['main_winding'][0]


def test_a_hand_built_fold():
    cnt, ef, et, pts = records(fold(), True)[:4]
    assert len(JR.join(ef, et)) == 1 and JR.join(ef, et)[0][1]                # the ring stays single
    ncross = [1, 1, 1, 1, 3, 3, 3, 1, 1, 1, 1, 1]
    lo = [3.5, 3.5, 3.5, 5.5, 1.5, 1.5, 1.5, 1.5, 3.5, 3.5, 3.5, 3.5]
    hi = [3.5, 3.5, 3.5, 5.5, 5.5, 5.5, 5.5, 1.5, 3.5, 3.5, 3.5, 3.5]
    for select in ('all', 'circumpolar', 'main'):
        out = run(fold(), True, select)
        expect(out, ncross, lo, hi)
        assert out['nsel'].tolist() == [1] and abs(int(out['main_winding'][0])) == 1 and out['main_nseg'][0] == cnt.sum()
    over = np.flatnonzero(out['ncross'][0] >= 3)
    assert over.tolist() == [4, 5, 6] and ((out['row_hi'] - out['row_lo'])[0, over] == 4.0).all()


def test_a_cut_off_blob_counts_under_all_only():
    with_blob = [1, 1, 1, 1, 1, 3, 1, 1, 1, 1, 1, 1]
    every = run(blob(), True, 'all')
    expect(every, with_blob, [3.5] * 5 + [0.5] + [3.5] * 6, [3.5] * NX)
    assert every['nsel'].tolist() == [2]
    for select in ('circumpolar', 'main'):
        out = run(blob(), True, select)
        expect(out, [1] * NX, [3.5] * NX, [3.5] * NX)
        assert out['nsel'].tolist() == [1]
    # the main ring is reported under every select, and is not the blob (whose ids are smaller)
    assert every['main_nseg'].tolist() == [NX] and every['main_first_edge'].tolist() == [2 * 3 * NX + 1]


def test_a_band_has_two_circumpolar_rings_and_main_picks_by_nseg_then_first_edge():
    out = run(band(False), True, 'circumpolar')
    expect(out, [2] * NX, [2.5] * NX, [4.5] * NX)
    assert out['nsel'].tolist() == [2]
    cnt, ef, et, pts = records(band(False), True)[:4]
    import cpiece_records_ref as RR
    (tab, _, _), = RR.pieces(cnt, ef, et, pts, NY, NX, np.arange(NY), np.arange(NX), True, float(NX))
    assert sorted(tab['winding'].tolist()) == [-1, 1] and tab['nseg'].tolist() == [NX, NX]
    # an exact tie of nseg: the smallest first_edge, the ring at 2.5
    tie = run(band(False), True, 'main')
    expect(tie, [1] * NX, [2.5] * NX, [2.5] * NX)
    assert (tie['nsel'].tolist(), tie['main_first_edge'].tolist(), tie['main_nseg'].tolist()) == ([1], [2 * 2 * NX + 1], [NX])
    # two more segments on the lower ring: it wins, though its first_edge is the larger one
    big = run(band(True), True, 'main')
    assert big['main_nseg'].tolist() == [NX + 2] and big['main_first_edge'].tolist() == [2 * 4 * NX + 1]
    assert big['main_winding'][0] == -tie['main_winding'][0]
    expect(big, [1] * NX, [4.5] * 6 + [5.5] + [4.5] * 5, [4.5] * 6 + [5.5] + [4.5] * 5)


def test_an_open_piece_on_a_plain_plane_counts_its_tail_once():
    out = run(step(4), False, 'all')
    expect(out, [1] * NX, [3.5] * NX, [3.5] * NX)                             # NX - 1 segments, NX vertices on vertical edges
    assert records(step(4), False)[0].sum() == NX - 1
    assert (out['nsel'].tolist(), out['main_first_edge'].tolist(), out['main_nseg'].tolist(), out['main_winding'].tolist()) == ([1], [-1], [0], [0])
    with pytest.raises(ValueError):
        run(step(4), False, 'main')


CASES = {'zonal': (lambda: step(4), True, 'main'), 'fold': (fold, True, 'main'), 'blob, main': (blob, True, 'main'),
         'blob, circumpolar': (blob, True, 'circumpolar'), 'band, tie': (lambda: band(False), True, 'main'),
         'band, bump': (lambda: band(True), True, 'main'), 'open': (lambda: step(4), False, 'all')}
# the case that catches each broken variant
CATCHES = {'e_to on rings': 'zonal', 'no selection': 'blob, main', 'first_edge only': 'band, bump', 'no fold': 'zonal'}


@pytest.mark.parametrize('wrong', OR.WRONG)
def test_every_wrong_variant_fails_a_case(wrong):
    failing = [name for name, (make, periodic, select) in CASES.items()
               if OR.differences(run(make(), periodic, select, wrong=wrong), run(make(), periodic, select))]
    assert CATCHES[wrong] in failing, '%s is caught by %r only' % (wrong, failing)


def test_the_wrong_variants_in_figures():
    """what each of them gives where it fails, by hand"""
    assert (run(step(4), True, 'main', wrong='e_to on rings')['ncross'] == 2).all()
    assert run(blob(), True, 'main', wrong='no selection')['ncross'][0, 5] == 3
    assert run(band(True), True, 'main', wrong='first_edge only')['main_nseg'].tolist() == [NX]
    nf = run(step(4), True, 'main', wrong='no fold')['ncross'][0]
    assert nf[:NX - 1].sum() == 0 and nf[NX - 1] == NX                       # V(3, c) has id >> 1 = 3 NX + c: every one past the row
    # and the tail of an open piece must not be dropped either
    cnt, ef, et, pts, ny, nx, per = records(step(4), False)
    starts_only = np.bincount((ef[ef & 1 == 1] >> 1) % nx, minlength=nx)
    assert starts_only.sum() == NX - 1 and run(step(4), False, 'all')['ncross'].sum() == NX
