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


# ------------------------------------------------------------------ the windows of the sums: the header's rule, stated and shown
import math

import cinside_sums_cases as SC
import cpiece_records_ref as RR
from test_gpu_cinside_records import SHAPES as RECORD_SHAPES, field, levels, scaled


def test_cut_drops_zeros_and_denormals_under_every_window():
    """a window's top is never below -800, its bottom never below -960: every zero and every denormal lies under it"""
    rng = np.random.default_rng(41)
    den = np.ldexp(rng.integers(1, 1 << 52, 200).astype(np.float64), -1074) * rng.choice([-1.0, 1.0], 200)
    den = np.concatenate([den, [5e-324, -5e-324, np.nextafter(2.0 ** -1022, 0.0), -np.nextafter(2.0 ** -1022, 0.0)]])
    assert (np.abs(den) < 2.0 ** -1022).all() and (den != 0.0).all()
    for bound in (0.0, 5e-324, 2.0 ** -1022, 2.0 ** -900, 2.0 ** -813, 2.0 ** -812, 1.0, 2.0 ** 1000, np.finfo(np.float64).max):
        top = RR.window_top(bound)
        assert top >= -800 and (bound < 2.0 ** -1022 or top == max(math.frexp(bound)[1] + 12, -800))
        for v in den.tolist() + [0.0, -0.0]:
            assert RR.cut(v, top - RR.WINDOW_BITS) == 0.0
        assert SC.same(IR.window_sum(den, top), 0.0) and SC.same(IR.window_sum([-0.0, -0.0], top), 0.0) and SC.same(IR.window_sum([], top), 0.0)
    assert RR.window_top(2.0 ** -813) == -800 and RR.window_top(2.0 ** -812) == -799 and RR.window_top(float('nan')) == -800
    # the smallest normal number under the lowest window: 2^-1022 is 62 bits under 2^-960
    assert RR.cut(2.0 ** -1022, -960) == 0.0 and RR.cut(2.0 ** -960, -960) == 2.0 ** -960 and RR.cut(1.5 * 2.0 ** -960, -960) == 2.0 ** -960
    assert math.isnan(IR.window_sum([1.0, np.inf, np.nan], 13)) and IR.window_sum([1.0, np.nan], 13) == 1.0


@pytest.mark.parametrize('shape', RECORD_SHAPES, ids=['%dx%d' % s for s in RECORD_SHAPES])
def test_on_the_scaled_inputs_of_the_records_suite_the_window_changes_nothing(shape):
    """exponents in [-20, 20]: every term lies wholly inside its window, so the sums of the header's rule ARE plain math.fsum, bit for
    bit -- what test_gpu_cinside_records.py asserted before the reference stated the window, it asserts still"""
    ny, nx = shape
    q = field(shape, 2, 50 + ny, nan=ny > 8)
    lv = levels(q, 3)
    rng = np.random.default_rng(60 + nx)
    w2, w3 = scaled(rng, (ny, nx)), scaled(rng, (2, ny, nx))
    f32, f64 = scaled(rng, (2, ny, nx), np.float32), scaled(rng, (2, ny, nx))
    w2[0, 0], f64[1, ny - 1, nx - 1] = np.nan, np.nan
    for periodic in (False, True):
        rec = (JP if periodic else JR).stack_records(q, lv) + (ny, nx, int(periodic))
        for w, f in ((w2, f64), (w3, f32), (None, None), (w2, None), (None, f64)):
            out = IR.interior(*rec, 'all', flip=1, ncont=3, w=w, f=f)
            for r, m in enumerate(out['mask'].astype(bool)):
                ws, wf = IR.slab_planes(w, f, r // 3, ny, nx)
                assert SC.same(out['sum_w'][r], IR.nan_skipping_sum(ws[m]))
                if f is not None:
                    assert SC.same(out['sum_wf'][r], IR.nan_skipping_sum(wf[m]))
                    assert all(RR.cut(t, out['tops'][r // 3][1] - 160) == t for t in wf[m & np.isfinite(wf)].tolist())
            assert all(-8 <= tw <= 33 and (tf is None or -28 <= tf <= 53) for tw, tf in out['tops'])
            assert out['n_in'].sum() > 0


def test_window_tops_per_slab_over_the_finite_values_of_all_of_the_plane():
    w = np.zeros((2, 3, 4))
    w[0, 0, 0], w[0, 1, 1], w[0, 2, 2] = -3.0, np.inf, np.nan                # |-3|: frexp exponent 2
    w[1, 2, 3] = 2.0 ** -30
    f = np.ones((2, 3, 4), dtype=np.float32)
    f[0, 0, 0], f[1, 2, 3], f[1, 0, 0] = 2.0 ** 20, -2.0 ** 5, np.inf       # 0 * inf: NaN, no bound
    assert IR.window_tops(w, f, 2, 3, 4) == [(14, 34), (-17, -12)]
    assert IR.window_tops(w[0], f, 2, 3, 4) == [(14, 34), (14, -800)]         # a shared plane: the same top_w; -3 * inf is no bound
    assert IR.window_tops(None, None, 2, 3, 4) == [(13, None), (13, None)] and IR.window_tops(None, f[:, :, :3], 1, 3, 3) == [(13, 33)]
    assert IR.window_tops(np.full((3, 4), np.nan), f, 1, 3, 4) == [(-800, -800)]
    big = np.full((3, 4), 2.0 ** 1000)
    assert IR.window_tops(big, np.full((1, 3, 4), 2.0 ** 100), 1, 3, 4) == [(1013, -800)]   # every product overflows: no finite value


def test_the_limb_model_on_k17s_windows_every_defect_caught_by_the_list_written_for_it():
    caught, seen = SC.limb_model_report('k17 rows')
    assert seen > 1000
    for d in RR.DEFECTS:
        assert SC.CATCHES[d] <= caught[d], (d, sorted(SC.CATCHES[d] - caught[d]))


@pytest.mark.parametrize('kind', SC.KINDS)
def test_three_broken_bound_rules_each_change_the_case_written_to_catch_it(kind):
    """on the planes of K17 and K18 alike (the bound is one pass, k_ci_bound, for both)"""
    B = SC.batches()
    pl = SC.plane(kind, 12, 70)
    # infinities counted into the bound: the window rises above every term
    cases = B['non-finite']
    W = SC.stack(pl, cases, 'strided')
    sw, _, _, tops = SC.reference(pl, len(cases), w=W)
    bad = IR.window_tops(W, None, len(cases), 12, 70, bound=SC.bound_with_infinities)
    assert [t[0] for t in tops] == [33] * 4 and [t[0] for t in bad] == [1036] * 4
    sw_bad = SC.reference(pl, len(cases), w=W, tops=bad)[0]
    assert np.isfinite(sw[0]) and sw[0] != 0.0 and sw_bad[0] == 0.0 and np.isnan(sw[1]) and np.isnan(sw[2]) and np.isfinite(sw[3])
    assert SC.same(sw[0], math.fsum(cases[0]['terms'])) and SC.same(sw[3], sw[0])       # exact; the NaN inside is skipped
    # the bound taken over the inside nodes alone: the far bound is not seen and nothing is cut
    cases = B['bound outside']
    W = SC.stack(pl, cases, 'strided')
    sw, _, _, tops = SC.reference(pl, 1, w=W)
    bad = IR.window_tops(W, None, 1, 12, 70, bound=SC.bound_over(pl['masks'][0]))
    assert tops == [(113, None)] and bad == [(-27, None)]
    sw_bad = SC.reference(pl, 1, w=W, tops=bad)[0]
    assert not SC.same(sw[0], sw_bad[0]) and SC.same(sw_bad[0], math.fsum(cases[0]['terms']))
    assert SC.same(sw[0], math.fsum(RR.cut(t, -47) for t in cases[0]['terms']))
    # the bound of w f taken from w: slab 0's products at 2^-60 lose the sticky bit under 2^(13 - 160)
    w, f, want_tops, want = SC.per_slab_case(pl, 'f')
    _, swf, _, tops = SC.reference(pl, 2, w=w, f=f)
    assert tops == want_tops and SC.same(swf, want)
    swf_bad = SC.reference(pl, 2, w=w, f=f, tops=[(tw, tw) for tw, _ in tops])[1]
    assert not SC.same(swf_bad[0], want[0]) and swf_bad[0] == 2.0 ** -60
    # ... and the windows of one slab used for the other (K17's mx[2 s] against mx[2 s + 1], s against r) show as well
    assert not SC.same(SC.reference(pl, 2, w=w, f=f, tops=tops[::-1])[1][0], want[0])
    w3, _, want_tops, want = SC.per_slab_case(pl, 'w')
    sw, _, _, tops = SC.reference(pl, 2, w=w3)
    assert tops == want_tops and SC.same(sw, want)


@pytest.mark.parametrize('kind', SC.KINDS)
def test_the_floor_the_float32_integrand_and_the_overflowing_product_differ_from_the_naive_expectation(kind):
    pl = SC.plane(kind, 12, 70)
    m = pl['masks'][0]
    for name, w, f, want in SC.floor_case(pl):
        sw, swf, n_in, tops = SC.reference(pl, 1, w=w, f=f)
        assert tops == [(-800, -800)] and n_in[0] == m.sum(), name
        assert SC.same(sw[0], want['sum_w']) and SC.same(swf[0], want['sum_wf']), name
        if 'NaN' not in name and 'zero' not in name:
            with np.errstate(all='ignore'):
                assert not SC.same(sw[0], math.fsum(w[m])) and not SC.same(swf[0], math.fsum((w * f[0])[m])), name    # the uncut sums
    w, f = SC.float32_integrand_case(pl)
    _, swf, _, _ = SC.reference(pl, 1, w=w, f=f)
    assert SC.same(swf[0], math.fsum((w * f[0].astype(np.float64))[m]))
    cast_after = (w * f[0].astype(np.float64)).astype(np.float32).astype(np.float64)
    in_float32 = (w.astype(np.float32) * f[0]).astype(np.float64)
    assert f.dtype == np.float32 and not SC.same(swf[0], math.fsum(cast_after[m])) and not SC.same(swf[0], math.fsum(in_float32[m]))
    for inside in (False, True):
        w, f = SC.overflow_case(pl, inside)
        sw, swf, _, tops = SC.reference(pl, 1, w=w, f=f)
        assert tops[0][0] == 1013 and 0 < tops[0][1] <= 53                   # the infinite product lifts no window
        assert np.isnan(swf[0]) == inside and SC.same(sw[0], 2.0 ** 1000 if inside else 0.0)
        if not inside:
            with np.errstate(all='ignore'):
                assert SC.same(swf[0], math.fsum((w * f[0])[m]))


def test_scan_geometry_of_the_records_suite_and_of_the_cuts_the_geometry_suite_adds():
    """the launch geometry of K17's scan as cinside_ref.scan_geometry restates it.  Every shape test_gpu_cinside_records.py runs has one
    column block (two on the hand-built 8 x 300, with two chunks), never the cap of 64 chunks, never a last chunk of one row;
    test_gpu_cinside_geometry.py asserts the regimes of its own shapes on the GPU machine, beside the runs"""
    G = IR.scan_geometry
    for shape in ((2, 2), (2, 65), (3, 64)):
        assert G(*shape, 6) == dict(ncb=1, nchunk=1, rc=shape[0], last=shape[0], wpr=(shape[1] + 31) // 32)
    for n in (2, 6, 140):
        assert G(9, 70, n) == dict(ncb=1, nchunk=2, rc=5, last=4, wpr=3)
        assert G(130, 7, n) == dict(ncb=1, nchunk=26, rc=5, last=5, wpr=1)
    for n in (6, 140):
        assert G(33, 130, n) == dict(ncb=1, nchunk=7, rc=5, last=3, wpr=5)
    assert G(8, 300, 5) == dict(ncb=2, nchunk=2, rc=4, last=4, wpr=10)
    # so many ranges that CI_BLOCKS = 4096 blocks are reached without cutting the rows
    assert G(130, 7, 4096)['nchunk'] == 1 and G(130, 7, 2048)['nchunk'] == 2
    assert (IR.CI_TPB, IR.CI_MIN_ROWS, IR.CI_MAX_CHUNKS, IR.CI_BLOCKS) == (256, 4, 64, 4096)
    assert G(256, 5, 1)['nchunk'] == 64 and G(261, 257, 2)['last'] == 1 and G(7, 513, 3)['nchunk'] == 1 and G(1025, 3, 1)['rc'] == 17
