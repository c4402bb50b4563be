"""xc_contour_distance_profile_dev (K28) at the limits of k_cd_profile and k_cd_profile_finish (cdprof_cases; test_cdprof_cases_host.py
shows on the CPU what each case holds): the LDS window at spans 1, 15, 16, 17 and 32 with all eight fields, so that the last word of a
full window and the counts behind it are written; edge tables of 512, 513 and 4097 edges with nodes ON the first, the last and three
inner edges and tiles of both kinds; per-slab weights and fields whose slabs lie 150 binary orders apart, three levels per slab; the
flags; bins that cancel to +0.0; the contour groups and slab batches of a signed call; planes around one tile column.

Through Context, so that `flags` is seen.  Everything on the Cartesian plane, where the device distance is the restatement's: EVERY
number is compared bit for bit (cdprof_ref.same_bits, np.array_equal), and tiles_window / tiles_global are EQUAL to
cdprof_cases.predict_tiles, which knows the distances alone.  Every case runs four ways -- as it stands, every tile on the global
words, one range per group, unpruned -- with the same bits.  Every call prints its counters."""
import numpy as np
import pytest

import cdist_ref as DR
import cdprof_cases as PC
import cdprof_ref as PR

pytestmark = pytest.mark.gpu

OUT = ('nodes', 'area', 'sums', 'flags')


def call(ctx, c):
    res = ctx.contour_distance_profile(c['q'], c['levels'], c['ycoord'], c['xcoord'], c['edges'], w=c['w'], fields=c['fields'],
                                       period=c['period'], select=c['select'], signed=c['signed'])
    return dict(zip(OUT, res))


def tiles(ctx):
    p = ctx.last_cdprofile_profile()
    return p['tiles_window'], p['tiles_global']


def same(a, b, what):
    for k in OUT:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), '%s: %s differs' % (what, k)


def check(got, e, what):
    """the call's four outputs against cdprof_cases.expected: integers equal, floats bit for bit, NaN exactly where the reference has it"""
    assert got['nodes'].dtype == np.int64 and np.array_equal(got['nodes'], e['nodes']), what + ': nodes'
    assert got['flags'].dtype == np.int32 and got['flags'].shape == e['flags'].shape and np.array_equal(got['flags'], e['flags']), what + ': flags'
    assert got['area'].dtype == np.float64 and PR.same_bits(got['area'], e['area']), what + ': area'
    assert got['sums'].dtype == np.float64 and got['sums'].shape == e['sums'].shape and PR.same_bits(got['sums'], e['sums']), what + ': sums'


def variants(ctx, c, what, predicted):
    """the call as it stands, with every tile on the global words, with one range per group and unpruned: the same bits, and the
    tiles of the window and of the global path as predicted from the distances -> the plain call's result"""
    got = call(ctx, c)
    plain = tiles(ctx)
    print('%s: tiles_window / tiles_global predicted %d / %d, reported %d / %d' % ((what,) + tuple(predicted) + plain))
    try:
        ctx.set_cdprofile_global(True)
        forced, t_forced = call(ctx, c), tiles(ctx)
        ctx.set_cdprofile_global(False)
        ctx.set_cpiece_workspace(1)
        one, t_one = call(ctx, c), tiles(ctx)
        ctx.set_cpiece_workspace(1 << 30)
        ctx.set_cdist_prune(False)
        un, t_un = call(ctx, c), tiles(ctx)
    finally:
        ctx.set_cdprofile_global(False)
        ctx.set_cpiece_workspace(1 << 30)
        ctx.set_cdist_prune(True)
    for o, name in ((forced, 'global path'), (one, 'one range per group'), (un, 'unpruned')):
        same(o, got, '%s, %s' % (what, name))
    assert plain == tuple(predicted), '%s: the window was chosen otherwise than span <= 16' % what
    assert t_forced == (0, sum(predicted)) and t_one == plain and t_un == plain, what
    return got, forced


def run(ctx, name):
    e = PC.expected(name)
    got, forced = variants(ctx, PC.case(name), name, e['tiles'])
    check(got, e, name)
    return PC.case(name), e, got, forced


# ------------------------------------------------------------------ 1. the window's span
@pytest.mark.parametrize('name', PC.RAMP)
def test_the_window_at_spans_1_15_16_17_and_32_with_eight_fields(ctx, name):
    """the ramp: the tile of rows 16 .. 31 of slab 0 spans exactly the bins the case is named for; 16 takes the window, 17 the global
    words (and its neighbour, at 16, the window)"""
    c, e, got, _ = run(ctx, name)
    span = int(name.split()[1])
    assert got['sums'].shape[2] == 8 and PC.tile_spans(c['dist'], c['edges'])[0, 1, 0] == span
    assert (e['tiles'][1] > 0) == (span > 16)


def test_a_full_window_its_last_word_and_the_counts_behind_it(ctx):
    """span 16, nf 8: the window's last word is word 4 of channel 8 of bin 15 of the tile, and the counts start right behind it.
    The tiles of rows 16 .. 31 and 32 .. 47 of slab 0 fill it: bins 15 .. 30 and 31 .. 46.  Then the same without fields."""
    c, e, got, _ = run(ctx, 'ramp 16')
    spans = PC.tile_spans(c['dist'], c['edges'])
    for top in (30, 46):
        assert spans[0, top // 16, 0] == 16 and e['nodes'][0, 0, top] == 20
        assert got['sums'][0, 0, 7, top].tobytes() == e['sums'][0, 0, 7, top].tobytes() and e['sums'][0, 0, 7, top] != 0.0
    assert np.array_equal(got['nodes'], e['nodes']) and got['nodes'][0, 0].tolist() == [40] + [20] * 46
    _, e0, got0, _ = run(ctx, 'ramp 16 nf0')
    assert got0['sums'].shape == (2, 1, 0, 47) and got0['flags'].shape == (2, 1, 1) and not got0['flags'].any()
    assert got0['area'].tobytes() == got['area'].tobytes() and np.array_equal(got0['nodes'], got['nodes'])


def test_the_smooth_plane_takes_both_paths_as_predicted(ctx):
    c, e, got, _ = run(ctx, 'smooth')
    assert e['tiles'][0] > 0 and e['tiles'][1] > 0 and got['sums'].shape[2] == 8


# ------------------------------------------------------------------ 2. the edge table
@pytest.mark.parametrize('name', PC.TABLES)
def test_edge_tables_of_512_513_and_4097_edges(ctx, name):
    """512 edges lie in LDS, 513 and 4097 are read through the cache -- by window tiles too (both counters > 0, as predicted); 4097
    take cdp_bin's 13 steps, and the nodes ON the last edge end at lo == nedge"""
    c, e, got, _ = run(ctx, name)
    assert e['tiles'][0] > 0 and e['tiles'][1] > 0
    assert np.array_equal(got['nodes'][..., 0], e['nodes'][..., 0]) and got['nodes'][..., 0].sum() > 0
    assert np.array_equal(got['nodes'][..., -1], e['nodes'][..., -1]) and got['nodes'][..., -1].sum() > 0
    assert int(got['nodes'].sum()) == c['dist'].size


# ------------------------------------------------------------------ 3. the per-slab index
def test_per_slab_weights_and_fields_150_binary_orders_apart(ctx):
    """three slabs of three levels, w and field 0 per slab and scaled by 2^-150, 1, 2^+150: a sum taken under another slab's top
    is flagged or loses bits (test_cdprof_cases_host.py).  Then the slabs of every input reversed: the output comes back reversed."""
    c, e, got, _ = run(ctx, 'magnitude')
    assert np.isfinite(e['area']).all() and np.isfinite(e['sums']).all()
    assert np.isfinite(got['area']).all() and np.isfinite(got['sums']).all() and not got['flags'].any()
    s = PC.swapped_slabs(c)
    back, _ = variants(ctx, s, 'magnitude, slabs reversed', e['tiles'])
    for k in OUT:
        assert back[k].tobytes() == np.ascontiguousarray(got[k][::-1]).tobytes(), 'slabs reversed: %s' % k


# ------------------------------------------------------------------ 4. flags and terms that are not finite
@pytest.mark.parametrize('name', ['ramp 16', 'ramp 17', 'smooth'])
def test_flags_are_set_by_infinite_terms_inside_bins_alone(ctx, name):
    """the whole flags array: a bit for the (range, channel) with an infinite term inside a bin -- field 4 --, none for the NaN of
    field 3 and none for the inf of field 5, which lies in no bin; the flagged bin of that channel is NaN and nothing else is"""
    c, e, got, _ = run(ctx, name)
    nslab, N = got['nodes'].shape[:2]
    assert np.array_equal(got['flags'], np.broadcast_to(np.array([0, 0, 0, 0, 0, 1, 0, 0, 0], dtype=np.int32), (nslab, N, 9)))
    for s in range(nslab):
        for k in range(N):
            b = PC.bin_of(c, s * N + k, c['at']['inf'])
            assert np.flatnonzero(np.isnan(got['sums'][s, k, 4])).tolist() == [b]
    assert np.isnan(got['sums']).sum() == nslab * N and np.isfinite(got['area']).all()


def test_an_infinite_weight_flags_the_area_and_skips_the_nan_product(ctx):
    """w = +inf at a node of slab 1 where field 6 is 0: the area and every other field of that bin are NaN and flagged; inf x 0 is
    NaN and skipped, so field 6 stays finite and unflagged; slab 0 is untouched"""
    c, e, got, _ = run(ctx, 'ramp 16 infw')
    b = PC.bin_of(c, 1, c['at']['zero'])
    assert got['flags'][1, 0].tolist() == [1, 1, 1, 1, 1, 1, 1, 0, 1] and got['flags'][0, 0].tolist() == [0, 0, 0, 0, 0, 1, 0, 0, 0]
    assert np.flatnonzero(np.isnan(got['area'][1, 0])).tolist() == [b] and np.isfinite(got['area'][0]).all()
    assert np.isfinite(got['sums'][1, 0, 6]).all() and got['sums'][1, 0, 6, b].tobytes() == e['sums'][1, 0, 6, b].tobytes()
    assert np.isnan(got['sums'][1, 0, [0, 1, 2, 3, 5, 7], b]).all()


# ------------------------------------------------------------------ 5. cancellation
@pytest.mark.parametrize('name', ['ramp 16', 'ramp 17'])
def test_bins_of_plus_minus_2k_pairs_return_plus_zero(ctx, name):
    """the pairs sit in different tile columns: the words cancel in memory, not in one window.  +0.0 by its bits, on the window path
    and on the global path ('ramp 17': rows 16 .. 31 of slab 0 take it unasked; then every tile is sent there)"""
    c, e, got, forced = run(ctx, name)
    zero = PC.cancelling_bins(e)
    assert zero.sum() >= 8 and zero[0, 0, 16:31].any()
    for res in (got, forced):
        z = np.ascontiguousarray(res['sums'][:, :, 2]).view(np.int64)
        assert (z[zero] == 0).all() and (res['area'][zero] != 0.0).all()
        assert (z[~zero & (e['nodes'] > 0)] != 0).all()


# ------------------------------------------------------------------ 6. groups and batches
def test_signed_contour_groups_and_slab_batches_give_the_single_calls_bits(ctx):
    """signed, select 'main', two slabs of three levels on the ring: under max_batch_bytes the contours go one, two and three at a
    time (K17's mask counts one byte per node and contour) and the slabs one per batch.  pairs_total of the LAST library call tells
    which ranges it held."""
    c, e = PC.case('ring'), PC.expected('ring')
    ny, nx = c['dist'].shape[1:]
    npl = ny * nx
    nsel = np.array([idx.size for idx, _ in DR.selected(*c['rec'], ny, nx, 1, PC.SELECT['main'])]).reshape(2, 3)
    assert (nsel > 0).all()
    got, _ = variants(ctx, c, 'ring', e['tiles'])
    check(got, e, 'ring')
    assert ctx.last_cdprofile_profile()['pairs_total'] == npl * nsel.sum()
    slab = npl * (8 + 4)                                                      # what a slab stages: q float64, field 1 float32
    keep = ctx.max_batch_bytes
    try:
        # (max_batch_bytes, the ranges of the last library call)
        for cap, last in ((npl, nsel[1, 2:]), (2 * npl, nsel[1, 2:]), (3 * npl, nsel[1]), (slab + 3 * npl, nsel[1]),
                          (2 * (slab + 3 * npl), nsel)):
            ctx.max_batch_bytes = cap
            part = call(ctx, c)
            same(part, got, 'max_batch_bytes %d' % cap)
            assert ctx.last_cdprofile_profile()['pairs_total'] == npl * last.sum(), cap
    finally:
        ctx.max_batch_bytes = keep


# ------------------------------------------------------------------ 7. the plane's edges
@pytest.mark.parametrize('name', PC.PLANES)
def test_planes_of_15_16_and_17_columns_and_a_one_row_tile_row(ctx, name):
    c, e, got, _ = run(ctx, name)
    assert (got['nodes'].sum(axis=-1) == c['dist'].shape[1] * c['dist'].shape[2]).all()
