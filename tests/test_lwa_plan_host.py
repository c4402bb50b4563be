"""lwa_plan_ref -- the restatement of K7's band-walk plan and of a wave's band that test_gpu_lwa_walk.py stands on -- pinned without a GPU:
walk_plan on a table worked out by hand from the LDS layout of k_lwa_strip, band on the oracle's own masks."""
import numpy as np
import pytest

import xcontour_oracle as O
import lwa_plan_ref as P

# ---------------------------------------------------------------- the LDS layout, by hand
# lwa_strip_lds: 6 [ny] double arrays = 48 ny bytes; the tracer strip [ny][65] = 520 ny (float64) or 260 ny (float32) bytes; 64 bytes for
# the union band; 512 wchunk bytes per staged plane (32768 / 16384 / 8192 for 64 / 32 / 16 rows).  So
#     float64: 568 ny + 64 + 512 wchunk planes        float32: 308 ny + 64 + 512 wchunk planes
# rounded up to a multiple of 16, against kLdsBudget = 150 * 1024 = 153600.
# (tsize, dA rank, M rank, wchunk, ny) -> bytes: the largest ny that fits and the first that does not, for every layout
LDS_TABLE = [
    # float64, weight and metric both planes (M absent is dA: a plane too): 568 ny + 64 + 1024 wchunk
    (8, 'plane', 'plane', 64, 154, 153072),    # 87472 + 65600                          fits
    (8, 'plane', 'plane', 64, 155, 153648),    # 88040 + 65600 = 153640 -> 153648      does not
    (8, 'plane', None, 32, 212, 153248),       # 120416 + 32832                         fits
    (8, 'plane', None, 32, 213, 153824),       # 120984 + 32832 = 153816 -> 153824     does not
    (8, 'plane', 'plane', 16, 241, 153344),    # 136888 + 16448 = 153336 -> 153344     fits
    (8, 'plane', 'plane', 16, 242, 153904),    # 137456 + 16448                         does not
    # float64, one plane (either of the two): 568 ny + 64 + 512 wchunk -- the byte counts of the line above, one chunk size up
    (8, 'plane', 'row', 64, 212, 153248),
    (8, 'row', 'plane', 64, 213, 153824),
    (8, 'row', 'plane', 32, 241, 153344),
    (8, 'plane', 'row', 32, 242, 153904),
    (8, 'plane', 'row', 16, 255, 153104),      # 144840 + 8256 = 153096 -> 153104      fits
    (8, 'row', 'plane', 16, 256, 153664),      # 145408 + 8256                          does not
    # float64, no plane: nothing is staged, 568 ny + 64 whatever the chunk
    (8, 'row', 'row', 64, 270, 153424),        # 153360 + 64                            fits
    (8, 'row', None, 16, 270, 153424),
    (8, 'row', None, 64, 271, 154000),         # 153928 + 64 = 153992 -> 154000        does not
    # float32, both planes: 308 ny + 64 + 1024 wchunk
    (4, 'plane', None, 64, 285, 153392),       # 87780 + 65600 = 153380 -> 153392      fits
    (4, 'plane', 'plane', 64, 286, 153696),    # 88088 + 65600 = 153688 -> 153696      does not
    (4, 'plane', 'plane', 32, 392, 153568),    # 120736 + 32832                         fits
    (4, 'plane', 'plane', 32, 393, 153888),    # 121044 + 32832 = 153876 -> 153888     does not
    (4, 'plane', 'plane', 16, 445, 153520),    # 137060 + 16448 = 153508 -> 153520     fits
    (4, 'plane', None, 16, 446, 153824),       # 137368 + 16448 = 153816 -> 153824     does not
    # float32, one plane: 308 ny + 64 + 512 wchunk
    (4, 'row', 'plane', 64, 392, 153568),
    (4, 'plane', 'row', 64, 393, 153888),
    (4, 'plane', 'row', 32, 445, 153520),
    (4, 'row', 'plane', 32, 446, 153824),
    (4, 'row', 'plane', 16, 471, 153328),      # 145068 + 8256 = 153324 -> 153328      fits
    (4, 'plane', 'row', 16, 472, 153632),      # 145376 + 8256                          does not
    # float32, no plane: 308 ny + 64
    (4, 'row', None, 64, 498, 153456),         # 153384 + 64 = 153448 -> 153456        fits
    (4, 'row', 'row', 64, 499, 153760),        # 153692 + 64 = 153756 -> 153760        does not
]


@pytest.mark.parametrize('tsize,da,m,wchunk,ny,want', LDS_TABLE)
def test_strip_lds_bytes_table(tsize, da, m, wchunk, ny, want):
    assert P.strip_lds_bytes(ny, tsize, *P.planes(da, m), wchunk) == want
    assert (want <= P.LDS_BUDGET) == (want <= 153600)


# (nslab, ny, nx, tsize, dA rank, M rank, keywords) -> plan.  nx = 130 is three strips; with two slabs and at most 63 workgroups per strip
# (ny <= 498) the grid has at most 378 workgroups: inside `few` on 256 CUs, so the LDS fit alone decides.
PLAN_TABLE = [
    # ---- the twelve limits with both planes (LDS_TABLE: the chunk that fits at each ny)
    (2, 154, 130, 8, 'plane', 'plane', {}, ('strip', 64)),
    (2, 155, 130, 8, 'plane', 'plane', {}, ('strip', 32)),
    (2, 212, 130, 8, 'plane', 'plane', {}, ('strip', 32)),
    (2, 213, 130, 8, 'plane', 'plane', {}, ('strip', 16)),
    (2, 241, 130, 8, 'plane', 'plane', {}, ('strip', 16)),
    (2, 242, 130, 8, 'plane', 'plane', {}, ('stream', 1)),       # 242^2 * 130 * 2 = 1.5e7
    (2, 285, 130, 4, 'plane', 'plane', {}, ('strip', 64)),
    (2, 286, 130, 4, 'plane', 'plane', {}, ('strip', 32)),
    (2, 392, 130, 4, 'plane', 'plane', {}, ('strip', 32)),
    (2, 393, 130, 4, 'plane', 'plane', {}, ('strip', 16)),
    (2, 445, 130, 4, 'plane', 'plane', {}, ('strip', 16)),
    (2, 446, 130, 4, 'plane', 'plane', {}, ('stream', 1)),       # 446^2 * 130 * 2 = 5.2e7
    # an absent metric is dA: with a plane dA both are planes, with a row dA none is
    (2, 154, 130, 8, 'plane', None, {}, ('strip', 64)),
    (2, 155, 130, 8, 'plane', None, {}, ('strip', 32)),
    (2, 445, 130, 4, 'plane', None, {}, ('strip', 16)),
    (2, 446, 130, 4, 'plane', None, {}, ('stream', 1)),
    # ---- one plane
    (2, 212, 130, 8, 'plane', 'row', {}, ('strip', 64)),
    (2, 213, 130, 8, 'plane', 'row', {}, ('strip', 32)),
    (2, 241, 130, 8, 'row', 'plane', {}, ('strip', 32)),
    (2, 242, 130, 8, 'row', 'plane', {}, ('strip', 16)),
    (2, 255, 130, 8, 'plane', 'row', {}, ('strip', 16)),
    (2, 256, 130, 8, 'plane', 'row', {}, ('stream', 1)),
    (2, 255, 130, 8, 'row', 'plane', {}, ('strip', 16)),
    (2, 256, 130, 8, 'row', 'plane', {}, ('stream', 1)),
    (2, 392, 130, 4, 'row', 'plane', {}, ('strip', 64)),
    (2, 393, 130, 4, 'row', 'plane', {}, ('strip', 32)),
    (2, 445, 130, 4, 'plane', 'row', {}, ('strip', 32)),
    (2, 446, 130, 4, 'plane', 'row', {}, ('strip', 16)),
    (2, 471, 130, 4, 'row', 'plane', {}, ('strip', 16)),
    (2, 472, 130, 4, 'row', 'plane', {}, ('stream', 1)),
    # ---- no plane: nothing is staged, the chunk reported is the 64 tried first
    (2, 270, 130, 8, 'row', None, {}, ('strip', 64)),
    (2, 271, 130, 8, 'row', None, {}, ('stream', 1)),
    (2, 270, 130, 8, 'row', 'row', {}, ('strip', 64)),
    (2, 271, 130, 8, 'row', 'row', {}, ('stream', 1)),
    (2, 498, 130, 4, 'row', 'row', {}, ('strip', 64)),
    (2, 499, 130, 4, 'row', None, {}, ('stream', 1)),
    # ---- the shapes the suite had before: all chunk 64 (the gap this table was written for), and the two reanalysis grids
    (1, 131, 70, 8, 'plane', None, {}, ('strip', 64)),
    (1, 256, 512, 4, 'plane', 'row', {}, ('strip', 64)),         # the barotropic field: 8 strips * 32 groups = 256 workgroups
    (1, 181, 360, 8, 'plane', 'row', {}, ('strip', 64)),         # 1 degree with a row metric: one plane
    (1, 181, 360, 8, 'plane', None, {}, ('strip', 32)),          #           with M = dA: two planes
    (1, 241, 480, 8, 'plane', None, {}, ('strip', 16)),          # 0.75 degree, one row under the limit: 8 * 31 = 248 workgroups
    (1, 241, 480, 8, 'row', 'row', {}, ('strip', 64)),
    # ---- `few`: strips * slabs * groups of 8 target rows <= 2 * CUs.  154 x 130: 3 * 20 = 60 workgroups per slab
    (8, 154, 130, 8, 'plane', 'plane', {}, ('strip', 64)),       # 480 <= 512
    (9, 154, 130, 8, 'plane', 'plane', {}, ('stream', 1)),       # 540;  154^2 * 130 * 9 = 2.8e7
    (9, 154, 130, 8, 'plane', 'plane', {'knob_strip': 2}, ('strip', 64)),      # XC_LWA_STRIP=2: at any grid size
    (1, 154, 130, 8, 'plane', 'plane', {'knob_strip': 0}, ('stream', 1)),      # XC_LWA_STRIP=0: never
    (1, 154, 130, 8, 'plane', 'plane', {'cus': 30}, ('strip', 64)),            # 60 <= 60
    (1, 154, 130, 8, 'plane', 'plane', {'cus': 29}, ('stream', 1)),
    (1, 154, 130, 8, 'plane', 'plane', {'cus': 0}, ('strip', 64)),             # an unknown CU count is 256
    (1, 8, 64 * 512, 8, 'row', None, {}, ('strip', 64)),         # 512 strips * 1 group
    (1, 9, 64 * 512, 8, 'row', None, {}, ('stream', 1)),         # 512 strips * 2 groups
    (1, 8, 64 * 512 + 1, 8, 'row', None, {}, ('stream', 1)),     # 513 strips
    # ---- the index limits of the strip kernel (32-bit offsets inside a plane); only XC_LWA_STRIP=2 gets that far
    (1, 100, 21474836, 8, 'row', None, {'knob_strip': 2}, ('strip', 64)),      # nx = (2^31 - 1) // 100
    (1, 100, 21474837, 8, 'row', None, {'knob_strip': 2}, ('stream', 4)),
    (65535, 16, 64, 8, 'row', None, {'knob_strip': 2}, ('strip', 64)),
    (65536, 16, 64, 8, 'row', None, {'knob_strip': 2}, ('stream', 4)),         # 256 * 64 * 65536 = 1.07e9
    # ---- one or four target rows per thread of k_lwa: ny^2 nx nslab against 2.0e8, `<` on the side of one
    (26, 242, 130, 8, 'plane', 'plane', {}, ('stream', 1)),      # 58564 * 130 = 7613320; * 26 = 197946320
    (27, 242, 130, 8, 'plane', 'plane', {}, ('stream', 4)),      #                        * 27 = 205559640
    (7, 446, 130, 4, 'row', 'plane', {'knob_strip': 0}, ('stream', 1)),        # 198916 * 130 = 25859080; * 7 = 181013560
    (8, 446, 130, 4, 'row', 'plane', {'knob_strip': 0}, ('stream', 4)),        #                          * 8 = 206872640
    (166, 131, 70, 8, 'plane', None, {'knob_strip': 0}, ('stream', 1)),        # 17161 * 70 = 1201270; * 166 = 199410820
    (167, 131, 70, 8, 'plane', None, {'knob_strip': 0}, ('stream', 4)),        #                       * 167 = 200612090
    (1, 1000, 199, 8, 'plane', None, {}, ('stream', 1)),         # 1.99e8
    (1, 1000, 200, 8, 'plane', None, {}, ('stream', 4)),         # 2.0e8 exactly: four
]


@pytest.mark.parametrize('nslab,ny,nx,tsize,da,m,kw,want', PLAN_TABLE)
def test_walk_plan_table(nslab, ny, nx, tsize, da, m, kw, want):
    assert P.walk_plan(nslab, ny, nx, tsize, da, m, **kw) == want


def test_walk_plan_refuses_what_the_prep_grid_cannot_hold():
    """xc_lwa.hip:106: blocks of 64 strips along grid z, 65535 at most"""
    assert P.walk_plan(1, 2, 64 * 64 * 65535, 8, 'row', None) == ('stream', 4)
    with pytest.raises(ValueError, match='nx too large'):
        P.walk_plan(1, 2, 64 * 64 * 65535 + 1, 8, 'row', None)


def test_largest_ny_and_smallest_stack_search_the_same_rule():
    assert P.largest_ny(('strip', 32), 2, 130, 8, 'plane', 'plane') == 212
    assert P.largest_ny(('strip', 16), 2, 130, 4, 'row', 'plane') == 471
    assert P.largest_ny(('strip', 64), 2, 130, 4, 'row', None) == 498
    assert P.smallest_stack(('stream', 4), 242, 130, 8, 'plane', 'plane') == 27
    assert P.smallest_stack(('stream', 4), 446, 130, 4, 'plane', 'plane') == 8


# ---------------------------------------------------------------- the band
def _field(dt, coord):
    rng = np.random.default_rng(77)
    ny, nx = coord.size, 70                                                # two strips, the second with 6 live columns
    q = (np.tanh(np.linspace(-3, 3, ny))[:, None] + 0.2 * np.sin(np.linspace(0, 6.28, nx))[None, :] + 0.02 * rng.standard_normal((ny, nx))).astype(dt)
    q[5, :] = np.nan                                                       # a row without a number: extrema +inf / -inf
    q[11, 3] = np.inf; q[20, 66] = -np.inf; q[14, :] = 0.1
    return q, rng


@pytest.mark.parametrize('coord', [np.linspace(-60, 60, 37), np.linspace(60, -60, 37), np.repeat(np.arange(19.0), 2)[:37]],
                         ids=['up', 'down', 'tied'])
@pytest.mark.parametrize('dt', [np.float64, np.float32])
def test_band_holds_every_row_of_the_oracles_mask(dt, coord):
    """band is a bound on where the oracle's mask3 (core.py:759-766 / 865-872), cut by `part` (core.py:773-784), is non-zero inside the
    strip: no row outside [y0, y1) has a kept cell, for both variants, both directions, every part, a sorted and an unsorted Q.  And
    the band is tight: its first and last rows passed lwa_row_needed, so each holds a kept cell.  bands == band row by row."""
    q, rng = _field(dt, coord)
    ny = coord.size
    dA = np.ones(q.shape)
    col = np.nan_to_num(q[:, 0].astype(np.float64), nan=0.0)
    for Q in (np.sort(col), rng.standard_normal(ny)):
        for variant, fn in ((0, O.cal_local_wave_activity), (1, O.cal_local_wave_activity2)):
            for increase in (True, False):
                with np.errstate(invalid='ignore'):
                    _, _, masks = fn(q.astype(np.float64), Q, coord, dA, increase, 'all', mask_idx=list(range(ny)))
                for part, name in enumerate(('all', 'upper', 'lower')):
                    for strip in (0, 1):
                        y0s, y1s = P.bands(q, Q, coord, increase, part, variant, strip)
                        for j in range(ny):
                            y0, y1 = P.band(q, Q, coord, increase, part, variant, j, strip)
                            assert (y0, y1) == (y0s[j], y1s[j])
                            m = masks[j][:, strip * 64:(strip + 1) * 64]
                            if name != 'all':
                                m = np.where((m > 0) if (name == 'upper') == increase else (m < 0), m, 0)
                            rows = np.flatnonzero((m != 0).any(axis=1))
                            if rows.size:
                                assert y0 <= rows[0] and rows[-1] < y1, (variant, increase, name, strip, j)
                            if y0 < y1:
                                assert (m[y0] != 0).any() and (m[y1 - 1] != 0).any(), (increase, name, strip, j)


def test_band_of_a_hand_built_strip():
    """3 columns; row values 0..5 in column 0 and the same + 0.5 in the others; Q = the row index; increasing coordinate and tracer.
    Target j: near rows y' >= j need a cell < Q[j] = j -- none (row y' holds y' and y' + 0.5 >= j); far rows y' < j need a cell > j:
    row y' = j - 1 holds j - 0.5, not more.  So every band is empty; with Q lowered by 1 the far rows j - 1 (j - 0.5 > j - 1) and j - 2
    (j - 1.5 < j - 1: no) give [j - 1, j), and the near side stays empty."""
    q = np.arange(6.0)[:, None] + np.array([0.0, 0.5, 0.5])[None, :]
    coord = np.arange(6.0)
    for j in range(6):
        assert P.band(q, np.arange(6.0), coord, True, 0, 0, j, 0) == (6, 0)
        want = (j - 1, j) if j >= 1 else (6, 0)
        assert P.band(q, np.arange(6.0) - 1.0, coord, True, 0, 0, j, 0) == want
        assert P.band(q, np.arange(6.0) - 1.0, coord, True, 2, 0, j, 0) == want          # 'lower' with increase: the far side
        assert P.band(q, np.arange(6.0) - 1.0, coord, True, 1, 0, j, 0) == (6, 0)        # 'upper': the near side, empty
        assert P.band(q, np.arange(6.0), coord, True, 0, 0, j, 1) == (6, 0)              # a strip past the plane: no number in it


def test_workgroups_counts_chunks_cuts_and_late_starts():
    ny = 20
    y0 = np.full(ny, ny); y1 = np.zeros(ny, dtype=np.int64)
    y0[0], y1[0] = 2, 5                   # workgroup 0: union [2, 19): with 4-row chunks 5 trips, boundaries at 6, 10, 14, 18
    y0[3], y1[3] = 7, 19                  #   wave 3 starts in the second chunk and is cut at 10, 14, 18
    y0[9], y1[9] = 4, 8                   # workgroup 1: one wave, one chunk
    w = P.workgroups(y0, y1, 4)           # workgroup 2 (rows 16..19): every band empty
    assert [g['union'] for g in w] == [(2, 19), (4, 8), (ny, 0)]
    assert [g['chunks'] for g in w] == [5, 1, 0]
    assert [g['cut'] for g in w] == [True, False, False]
    assert [g['late'] for g in w] == [True, False, False]
    y0[3], y1[3] = 6, 10                  # starts ON a boundary and ends on the next: late, not cut
    w = P.workgroups(y0, y1, 4)
    assert w[0]['union'] == (2, 10) and w[0]['chunks'] == 2 and w[0]['late'] and not w[0]['cut']
