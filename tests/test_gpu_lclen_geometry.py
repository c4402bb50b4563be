"""K11 (xc_lclen.hip, xc_local_contour_lengths) on every window geometry: each of the three block-level loops of lclen_window in more
than one round, both block sizes, the strip edges, the ring.

The loops: the mean `for (b = 0; b < wh; b += ntd)` (a second round needs more than 64 / 256 node rows), the carry
`for (s0 = 0; s0 < nstrip; s0 += nwave * 31)` (a second round needs more than 31 / 124 strips of 16 x 64 cells) and the block-size
rule `cells of the unclipped window <= 2048 ? 64 : 256`.  No launch record exists for K11, so every case states the side it means
to sit on through local_clength_ref.launch_shape -- the rule restated -- and fails when its shape drifts.

Checked like test_gpu_local_contour_lengths: levels bit for bit against the restatement (NaN where it has NaN), counts exact, totals
within 1e-12 (the project's K11 / K10 bound against this restatement), NaN lengths exactly where it has them.  Where every length
is exact (fields that vary along x only on few-bit coordinates) the totals are the fixed-point model det_window_total bit for bit.
Every case also asserts that its target window has segments and -- except where min_periods is meant to fail -- that at least half
of the windows of the call have a contour."""
import numpy as np
import pytest

import clength_periodic_ref as PR
import clength_ref as CR
import local_clength_ref as LR
from test_gpu_local_contour_lengths import bits_equal, check, coords, field
from test_gpu_periodic_contour_lengths import _k11_identity, dyadic, hashed_plane

pytestmark = pytest.mark.gpu

DY, DX = 0.75, 0.5                                           # the uniform spacing of the closed forms (dyadic: coordinates exact)


# ------------------------------------------------------------------ helpers
def same_bits(a, b):
    """NaN at the same places, the same bits everywhere else (a NaN's payload is not part of any rule)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na = np.isnan(a)
    return a.shape == b.shape and np.array_equal(na, np.isnan(b)) and bits_equal(a[~na], b[~na])


def extents(window, plane, stride, ring=False):
    """-> (node rows of every window row (nwy,), node columns of every window column (nwx,)) after clipping; a ring does not clip X"""
    (r0, r1), (c0, c1) = LR.bounds(plane[0], window[0], stride[0]), LR.bounds(plane[1], window[1], stride[1])
    return r1 - r0 + 1, (np.full(c0.size, window[1]) if ring else c1 - c0 + 1)


def cells(window, plane, stride, ring=False):
    """-> (nwy, nwx) cells of every window"""
    rows, cols = extents(window, plane, stride, ring)
    return np.outer(rows - 1, cols - 1)


def shape_at(window, plane, stride, at, ring=False, unclipped=True):
    """launch_shape of window `at`; asserts that the window is not clipped (unless told that it is)"""
    rows, cols = extents(window, plane, stride, ring)
    r, c = int(rows[at[0]]), int(cols[at[1]])
    assert ((r, c) == tuple(window)) == unclipped, (window, plane, at, r, c)
    return LR.launch_shape(window, plane, r, c)


def checkerboard(plane, dt=np.float64):
    """+-1 in a checkerboard: at level 0.0 every cell is a saddle with two segments between the mid points of its sides"""
    return (np.indices(plane).sum(0) % 2 * 2.0 - 1.0).astype(dt)


def uniform_coords(plane):
    return 3.0 + DY * np.arange(plane[0]), -1.0 + DX * np.arange(plane[1])


def make(kind, plane, seed, dt=np.float64):
    return checkerboard(plane, dt) if kind == 'checker' else field(kind, plane, seed, dt)


def run(ctx, q2d, y, x, window, stride, latlon, mp=1, levels=None, period=None, at=None, dense=True, what=''):
    """one slab, one call, against the restatement (periodic: clength_periodic_ref) on the levels the GPU returned
    -> (lengths, levels, counts, restated totals), each (nwy, nwx)"""
    lens, lvls, cnts = ctx.local_contour_lengths(np.ascontiguousarray(q2d[None]), y, x, window, stride, mp, levels=levels,
                                                 radius=CR.RADIUS if latlon else 0.0, period=period)
    lens, lvls, cnts = lens[0], lvls[0], cnts[0].astype(np.int64)
    q64 = q2d.astype(np.float64)
    if levels is not None:
        ref = np.broadcast_to(np.asarray(levels, dtype=np.float64), lvls.shape)
    elif period is None:
        ref = LR.window_levels(q64, window, stride, mp)
    else:
        ref = PR.window_levels(q64, window, stride, period, mp)
    assert same_bits(lvls, ref), '%s: levels' % what
    if period is None:
        rt, rn = LR.local_contour_lengths(q64, lvls, y, x, window, stride, latlon)
    else:
        rt, rn = PR.local_contour_lengths(q64, lvls, y, x, period, window, stride, latlon)
    check(lens, cnts, rt, rn, what)
    if at is not None:
        assert rn[at] > 0, '%s: the target window has no segments' % what
    if dense:
        assert (rn > 0).mean() >= 0.5, '%s: %d of %d windows have a contour' % (what, (rn > 0).sum(), rn.size)
    return lens, lvls, cnts, rt


def run_checkerboard(ctx, plane, window, stride, latlon, dt, at, period=None):
    """level 0.0 on the checkerboard: two segments in every cell; on uniform planar spacing each is hypot(dx, dy) / 2 long"""
    q = checkerboard(plane, dt)
    nc = cells(window, plane, stride, period is not None)
    trials = [coords(plane[0], plane[1], latlon)] + ([] if latlon else [uniform_coords(plane)])
    for k, (y, x) in enumerate(trials):
        lens, _, cnts, _ = run(ctx, q, y, x, window, stride, latlon, levels=0.0, at=at, what='checkerboard %r' % (window,))
        assert np.array_equal(cnts, 2 * nc)
        if k == 1:
            want = nc[nc > 0] * np.hypot(DX, DY)
            assert np.max(np.abs(lens[nc > 0] - want) / want) <= 1e-12
            assert np.isnan(lens[nc == 0]).all()


# ------------------------------------------------------------------ (a) one wave, the carry twice
A_PLANE, A_STRIDE, A_AT = (6, 2100), (1, 1050), (3, 1)                   # centre column 1050: columns 26 .. 2074, not clipped
A_WINDOWS = [((2, 2049), (64, 1, 32, 2)),                                # 1 x 2048 cells: one wave, 31 strips and one more
             ((2, 2050), (256, 1, 33, 1))]                               # 2049 cells: four waves, one round


@pytest.mark.parametrize('latlon', [False, True])
@pytest.mark.parametrize('dt', [np.float32, np.float64])
@pytest.mark.parametrize('kind', ['random', 'nan', 'checker'])
@pytest.mark.parametrize('window,want', A_WINDOWS)
def test_a_one_wave_carries_twice(ctx, window, want, kind, dt, latlon):
    assert shape_at(window, A_PLANE, A_STRIDE, A_AT) == want
    if kind == 'checker':
        run_checkerboard(ctx, A_PLANE, window, A_STRIDE, latlon, dt, A_AT)
        return
    y, x = coords(A_PLANE[0], A_PLANE[1], latlon)
    run(ctx, make(kind, A_PLANE, 3, dt), y, x, window, A_STRIDE, latlon, at=A_AT, what='a %s %r' % (kind, window))


# ------------------------------------------------------------------ (b) one wave, the mean in up to three rounds
B_PLANE, B_STRIDE = (200, 9), (1, 4)
B_WINDOWS = [((150, 5), {128, 129, 150}, {2, 3}),                        # window, node rows that must occur, the mean rounds they take
             ((128, 5), {64, 65, 128}, {1, 2})]


@pytest.mark.parametrize('latlon', [False, True])
@pytest.mark.parametrize('dt', [np.float32, np.float64])
@pytest.mark.parametrize('window,heights,rounds', B_WINDOWS)
def test_b_one_wave_mean_in_rounds(ctx, window, heights, rounds, dt, latlon):
    rows, cols = extents(window, B_PLANE, B_STRIDE)
    assert heights <= set(rows.tolist()) and int(cols[1]) == window[1]
    shapes = [LR.launch_shape(window, B_PLANE, int(r), window[1]) for r in rows]
    assert {s[0] for s in shapes} == {64} and {s[1] for s in shapes} == rounds and {s[3] for s in shapes} == {1}
    assert max(s[2] for s in shapes) == -(-(window[0] - 1) // 16) and (150 - 1) % 16 == 5     # (150, 5): ten row strips, the last of 5 rows
    at = (int(np.argmax(rows == window[0])), 1)
    y, x = coords(B_PLANE[0], B_PLANE[1], latlon)
    run(ctx, make('random', B_PLANE, 4, dt), y, x, window, B_STRIDE, latlon, at=at, what='b random %r' % (window,))
    q = make('nan', B_PLANE, 5, dt)
    _, lv, _, _ = run(ctx, q, y, x, window, B_STRIDE, latlon, at=at, what='b nan %r' % (window,))
    assert not np.isnan(lv).any()
    # the valid count decides: the full window (every window misses it: clipped, or with a NaN) and the median count (both outcomes)
    (r0, r1), (c0, c1) = LR.bounds(B_PLANE[0], window[0], B_STRIDE[0]), LR.bounds(B_PLANE[1], window[1], B_STRIDE[1])
    valid = np.array([[(~np.isnan(q[a:b + 1, c:d + 1])).sum() for c, d in zip(c0, c1)] for a, b in zip(r0, r1)])
    _, lv, _, _ = run(ctx, q, y, x, window, B_STRIDE, latlon, mp=window[0] * window[1], dense=False, what='b nan full')
    assert valid.max() < window[0] * window[1] and np.isnan(lv).all()
    mid = int(np.median(valid))
    _, lv, _, _ = run(ctx, q, y, x, window, B_STRIDE, latlon, mp=mid, dense=False, what='b nan median')
    assert np.array_equal(np.isnan(lv), valid < mid) and 0 < np.isnan(lv).sum() < lv.size


# ------------------------------------------------------------------ (c) four waves, the mean in two rounds
@pytest.mark.parametrize('latlon', [False, True])
@pytest.mark.parametrize('kind', ['random', 'nan'])
def test_c_four_waves_mean_in_two_rounds(ctx, kind, latlon):
    plane, stride, window = (330, 14), (1, 7), (300, 12)
    rows, cols = extents(window, plane, stride)
    assert {150, 256, 257, 300} <= set(rows.tolist()) and int(cols[1]) == 12 and shape_at(window, plane, stride, (150, 1)) == (256, 2, 19, 1)
    shapes = [LR.launch_shape(window, plane, int(r), 12) for r in rows]
    assert {s[:2] for s in shapes} == {(256, 1), (256, 2)}
    y, x = coords(plane[0], plane[1], latlon)
    run(ctx, make(kind, plane, 6), y, x, window, stride, latlon, at=(150, 1), what='c %s' % kind)


# ------------------------------------------------------------------ (d) four waves at and past the capacity of a copy
D_PLANE, D_STRIDE, D_AT = (70, 2100), (35, 1050), (1, 1)
D_WINDOWS = [((65, 1985), (256, 1, 124, 1), True),                       # 64 x 1984 cells: 31 full strips in every wave, 31744 cells a copy
             ((65, 1986), (256, 1, 128, 2), True),                       # one cell column more: the second round's strips hold one lane
             ((81, 1985), (256, 1, 155, 2), False)]                      # taller than the plane (70 rows): 5 x 31 strips
D_FIELDS = [('checker', np.float64), ('random', np.float64), ('random', np.float32), ('nan', np.float64)]


@pytest.mark.parametrize('latlon', [False, True])
@pytest.mark.parametrize('kind,dt', D_FIELDS, ids=['%s-%s' % (k, np.dtype(d).name) for k, d in D_FIELDS])
@pytest.mark.parametrize('window,want,unclipped', D_WINDOWS)
def test_d_four_waves_at_and_past_the_copy_capacity(ctx, window, want, unclipped, kind, dt, latlon):
    assert shape_at(window, D_PLANE, D_STRIDE, D_AT, unclipped=unclipped) == want
    if kind == 'checker':
        run_checkerboard(ctx, D_PLANE, window, D_STRIDE, latlon, dt, D_AT)
        return
    y, x = coords(D_PLANE[0], D_PLANE[1], latlon)
    run(ctx, make(kind, D_PLANE, 7, dt), y, x, window, D_STRIDE, latlon, at=D_AT, what='d %s %r' % (kind, window))


# ------------------------------------------------------------------ (e) the fixed-point rule through the carry, bit for bit
E_ROWS = [(A_PLANE, A_STRIDE, A_AT, w, s, True) for w, s in A_WINDOWS] + [(D_PLANE, D_STRIDE, D_AT, w, s, u) for w, s, u in D_WINDOWS]


def x_profile(nx, how, seed):
    """the node values along x: 'sorted' (as K10's fixed-point test: a level crosses one cell column) or 'zigzag' (unsorted: a level
    crosses about every second cell, so the sums really run through the carry); some flat sides"""
    prof = np.random.default_rng(seed).uniform(-3.0, 3.0, nx)
    if how == 'sorted':
        prof.sort()
    prof[::17] = prof[1::17][:prof[::17].size]
    return prof


def window_levels_on(prof, window, plane, stride, how, seed):
    """a level per window that its columns cross: between two of its nodes, or (every third window) on a node value"""
    rng = np.random.default_rng(seed)
    c0, c1 = LR.bounds(plane[1], window[1], stride[1])
    nwy = LR.centres(plane[0], stride[0]).size
    lv = np.empty((nwy, c0.size))
    for j in range(nwy):
        for i in range(c0.size):
            k = int(rng.integers(c0[i] + 1, c1[i] - 1))
            lv[j, i] = prof[k] if (j + i) % 3 == 0 else 0.5 * (prof[k] + prof[k + 1])
            if how == 'zigzag' and (j + i) % 3:
                lv[j, i] = rng.uniform(-1.0, 1.0)
    return lv


def fixed_point_case(ctx, plane, stride, window, how, y, x):
    prof = x_profile(plane[1], how, len(how) + window[1])
    q = np.broadcast_to(prof[None, :], plane).copy()
    lv = window_levels_on(prof, window, plane, stride, how, window[0])
    lens, lvls, cnts = ctx.local_contour_lengths(q[None], y, x, window, stride, 1, levels=lv)
    lens, cnts = lens[0], cnts[0].astype(np.int64)
    assert bits_equal(lvls[0], lv)
    rt, rn = LR.local_contour_lengths(q, lv, y, x, window, stride)
    assert np.array_equal(cnts, rn) and (rn > 0).mean() >= 0.5
    model = np.array([[LR.det_window_total(q, lv[j, i], y, x, window, stride, j, i) for i in range(lv.shape[1])]
                      for j in range(lv.shape[0])])
    assert np.array_equal(np.isnan(lens), np.isnan(model))
    ok = ~np.isnan(model)
    assert bits_equal(lens[ok], model[ok]), 'fixed-point rule: max ulp %d' % np.max(np.abs(lens[ok].view(np.int64) - model[ok].view(np.int64)))
    return lens, cnts, rt, rn, model


@pytest.mark.parametrize('how', ['sorted', 'zigzag'])
@pytest.mark.parametrize('plane,stride,at,window,want,unclipped', E_ROWS, ids=['%dx%d' % r[3] for r in E_ROWS])
def test_e_fixed_point_rule_through_the_carry(ctx, plane, stride, at, window, want, unclipped, how):
    """Segments along y only: every length is one y spacing, exactly (the premise of K10's test_fixed_point_rule_bit_for_bit), so a
    window's total is the fixed-point model of its segments -- whatever the strips, the waves and the carry rounds did to the order"""
    assert shape_at(window, plane, stride, at, unclipped=unclipped) == want
    y, x = CR.few_bits(plane[0], 1, 1.0), CR.few_bits(plane[1], 2, 1.0)
    lens, cnts, rt, rn, _ = fixed_point_case(ctx, plane, stride, window, how, y, x)
    check(lens, cnts, rt, rn, 'e %s %r' % (how, window))
    assert rn[at] > 0 and (how == 'sorted' or rn[at] > cells(window, plane, stride)[at] // 4)


@pytest.mark.parametrize('plane,stride,at,window,want,wide_from', [(A_PLANE, A_STRIDE, A_AT) + A_WINDOWS[0] + (2080,),
                                                                    (D_PLANE, D_STRIDE, D_AT) + D_WINDOWS[1][:2] + (2060,)], ids=['a', 'd'])
def test_e_wide_cell_outside_every_window(ctx, plane, stride, at, window, want, wide_from):
    """one cell 2^120 times the others, in columns no window of the call owns: the window constant is the whole plane's, so the short
    segments (2^-44) lose their low bits under the window -- the model built on the plane's bound drops the same bits, a plain sum of
    the window's segments does not"""
    assert shape_at(window, plane, stride, at) == want
    c0, c1 = LR.bounds(plane[1], window[1], stride[1])
    assert c1.max() < wide_from - 1
    y, x = CR.few_bits(plane[0], 1, 2.0 ** -44), CR.few_bits(plane[1], 2, 1.0)
    x[wide_from:] += 2.0 ** 120
    lens, cnts, rt, rn, model = fixed_point_case(ctx, plane, stride, window, 'zigzag', y, x)
    assert rn[at] > cells(window, plane, stride)[at] // 4
    assert model[at] != rt[at] and lens[at] != rt[at], 'the wide cell must cost the short segments bits'


# ------------------------------------------------------------------ (f) strip edges
@pytest.mark.parametrize('latlon', [False, True])
@pytest.mark.parametrize('kind', ['node', 'nan'])
def test_f_strip_edges(ctx, kind, latlon):
    """cell heights 15 / 16 / 17 (one row strip, exactly one, one and a row) x cell widths 63 / 64 / 65 / 128 / 129 (a lane short of a
    strip, full lanes, one lane in the next), on both sides of the 2048 cells of the block-size rule"""
    plane, stride, at = (40, 300), (10, 50), (2, 3)                      # centre (20, 150): not clipped for any of the windows
    y, x = coords(plane[0], plane[1], latlon)
    q = make(kind, plane, 8)
    seen = set()
    for wy in (16, 17, 18):
        for wx in (64, 65, 66, 129, 130):
            threads, mean_rounds, strips, carries = shape_at((wy, wx), plane, stride, at)
            assert threads == (64 if (wy - 1) * (wx - 1) <= 2048 else 256) and (mean_rounds, carries) == (1, 1)
            assert strips == (1 if wy <= 17 else 2) * (1 if wx <= 65 else 2 if wx <= 129 else 3)
            seen.add(threads)
            if kind == 'node':                                            # levels on node values, given per window
                nw = cells((wy, wx), plane, stride).shape
                lv = np.random.default_rng(wy * wx).integers(1, 5, size=nw).astype(np.float64)
                run(ctx, q, y, x, (wy, wx), stride, latlon, levels=lv, at=at, what='f node %dx%d' % (wy, wx))
            else:
                run(ctx, q, y, x, (wy, wx), stride, latlon, at=at, what='f nan %dx%d' % (wy, wx))
    assert seen == {64, 256}


# ------------------------------------------------------------------ (g) the same window under both block sizes
@pytest.mark.parametrize('latlon', [False, True])
@pytest.mark.parametrize('kind', ['random', 'nan'])
def test_g_same_window_both_block_sizes(ctx, kind, latlon):
    """window (33, 65) centred on row 16 and window (35, 65) centred on row 15 own the same nodes, rows 0 .. 32 and columns 0 .. 64;
    the first launches 64 threads (32 x 64 = 2048 cells), the second 256 (34 x 64 unclipped): the header's promise is the same bits"""
    plane, stride = (40, 70), (1, 32)
    small, large = ((33, 65), (16, 1)), ((35, 65), (15, 1))
    assert shape_at(small[0], plane, stride, small[1]) == (64, 1, 2, 1)
    assert shape_at(large[0], plane, stride, large[1], unclipped=False) == (256, 1, 2, 1)
    for (w, at) in (small, large):
        (r0, r1), (c0, c1) = LR.bounds(plane[0], w[0], 1), LR.bounds(plane[1], w[1], 32)
        assert (r0[at[0]], r1[at[0]], c0[at[1]], c1[at[1]]) == (0, 32, 0, 64)
    y, x = coords(plane[0], plane[1], latlon)
    q = make(kind, plane, 9)
    for lv in (None, 0.1):
        a = run(ctx, q, y, x, small[0], stride, latlon, levels=lv, at=small[1], what='g 64 threads')
        b = run(ctx, q, y, x, large[0], stride, latlon, levels=lv, at=large[1], what='g 256 threads')
        for u, v in zip(a[:3], b[:3]):                                    # lengths, levels, counts
            assert not np.isnan(u[small[1]]) and bits_equal(np.float64(u[small[1]]), np.float64(v[large[1]])), lv


# ------------------------------------------------------------------ (h) the whole plane as one window, four carry rounds
@pytest.mark.parametrize('latlon', [False, True])
def test_h_whole_plane_in_four_carry_rounds_is_k10(ctx, latlon):
    plane = (600, 700)
    window, stride = (2 * plane[0], 2 * plane[1]), plane                 # one centre, node (0, 0): the whole plane after clipping
    assert shape_at(window, plane, stride, (0, 0), unclipped=False) == (256, 3, 418, 4)
    assert [v.tolist() for v in extents(window, plane, stride)] == [[600], [700]]
    y, x = coords(plane[0], plane[1], latlon)
    q = make('random', plane, 21)
    radius = CR.RADIUS if latlon else 0.0
    for lv in (0.3, -1.1):
        lens, _, cnts, _ = run(ctx, q, y, x, window, stride, latlon, levels=lv, at=(0, 0), what='h whole plane')
        k10, n10 = ctx.contour_lengths(q[None], [lv], y, x, radius=radius)
        assert cnts[0, 0] == n10[0, 0]
        # the header of xc_lclen.hip: K10's fixed-point sums on K10's window constant -- the same integers, converted once
        assert bits_equal(lens[0, 0], k10[0, 0]), (lens[0, 0], k10[0, 0])


# ------------------------------------------------------------------ (i) the ring
def dyadic_ring(ny, nx, latlon):
    """-> (y, x, period) of few-bit values: x +- period is exact and the window constant that of the tiled plane.  Sphere: latitude
    descending within (-pi/2, pi/2) for up to 200 rows, longitude below 2.1 for up to 2100 columns"""
    if latlon:
        y, x = dyadic(ny, 1, 2.0 ** -9, start=-1.25, descending=True), dyadic(nx, 2, 2.0 ** -12)
        assert y.min() > -1.5 and x.max() < 2.1
        return y, x, float(x[-1] - x[0] + 3 * 2.0 ** -12)
    y, x = dyadic(ny, 3, 0.5, start=5.0), dyadic(nx, 4, 0.25, start=-3.0)
    return y, x, float(x[-1] - x[0] + 0.75)


I_ROWS = [('a', A_PLANE, (2, 2049), A_STRIDE, (3, 0), {(64, 1, 32, 2)}),                 # centre column 0: columns -1024 .. 1024
          ('b', B_PLANE, (150, 5), B_STRIDE, (75, 0), {(64, 2), (64, 3)}),               # the modulo path of the mean, in rounds
          ('d', D_PLANE, (65, 1986), D_STRIDE, (1, 0), {(256, 1, 128, 2)})]


@pytest.mark.parametrize('latlon', [False, True])
@pytest.mark.parametrize('kind', ['random', 'nan'])
@pytest.mark.parametrize('name,plane,window,stride,at,want', I_ROWS, ids=[r[0] for r in I_ROWS])
def test_i_ring(ctx, name, plane, window, stride, at, want, kind, latlon):
    rows, cols = extents(window, plane, stride, ring=True)
    assert (cols == window[1]).all() and window[1] <= plane[1] and int(rows[at[0]]) == window[0]
    shapes = {LR.launch_shape(window, plane, int(r), window[1]) for r in rows if name == 'b' or r == window[0]}
    assert {s[:len(next(iter(want)))] for s in shapes} == want
    ny, nx = plane
    q = make(kind, plane, 10)
    y, x, period = hashed_plane(ny, nx, latlon)
    run(ctx, q, y, x, window, stride, latlon, period=period, at=at, what='i %s %s' % (name, kind))
    # the existing identity on few-bit coordinates: the periodic call is the plain kernel on the tiled plane, bit for bit
    y, x, period = dyadic_ring(ny, nx, latlon)
    got = _k11_identity(ctx, q[None], y, x, period, window, stride, 1, CR.RADIUS if latlon else 0.0)
    assert got[2][0][at] > 0 and (got[2][0] > 0).mean() >= 0.5


# ------------------------------------------------------------------ (j) small rules
J_ROWS = [((20, 22), (5, 5), (2, 5), (2, 1), (slice(2, 7), slice(3, 8)), 64),            # window (2, 1): rows 2 .. 6, columns 3 .. 7
          ((100, 110), (47, 47), (25, 55), (1, 1), (slice(2, 49), slice(32, 79)), 256)]  # window (1, 1): rows 2 .. 48, columns 32 .. 78


@pytest.mark.parametrize('plane,window,stride,at,patch,threads', J_ROWS, ids=['one-wave', 'four-waves'])
def test_j_min_periods_zero_on_an_all_nan_window(ctx, plane, window, stride, at, patch, threads):
    assert shape_at(window, plane, stride, at)[0] == threads
    q = make('random', plane, 12)
    q[patch] = np.nan
    y, x = coords(plane[0], plane[1], False)
    (r0, r1), (c0, c1) = LR.bounds(plane[0], window[0], stride[0]), LR.bounds(plane[1], window[1], stride[1])
    assert np.isnan(q[r0[at[0]]:r1[at[0]] + 1, c0[at[1]]:c1[at[1]] + 1]).all()
    lens, lvls, cnts, _ = run(ctx, q, y, x, window, stride, False, mp=0, what='j mp=0')          # 0 / 0: a NaN level
    assert np.isnan(lvls[at]) and np.isnan(lens[at]) and cnts[at] == 0
    assert np.isnan(lvls).sum() == 1
    one = run(ctx, q, y, x, window, stride, False, mp=1, what='j mp=1')                          # the neighbours are not affected
    for u, v in zip((lens, lvls, cnts), one[:3]):
        assert same_bits(u, v)


@pytest.mark.parametrize('plane,window,stride,at,patch,threads', J_ROWS, ids=['one-wave', 'four-waves'])
def test_j_a_window_of_negative_zeros_has_the_level_plus_zero(ctx, plane, window, stride, at, patch, threads):
    """the mean starts from 0.0 (the header of xc_lclen.hip): 0.0 + -0.0 is +0.0, a sum is never -0.0"""
    assert shape_at(window, plane, stride, at)[0] == threads
    y, x = coords(plane[0], plane[1], False)
    for with_nan in (False, True):
        q = make('random', plane, 13)
        q[patch] = -0.0
        if with_nan:
            q[patch][::2, 1::3] = np.nan
            assert np.isnan(q[patch]).sum() > 3
        _, lvls, cnts, _ = run(ctx, q, y, x, window, stride, False, mp=1, what='j -0.0')
        assert lvls[at] == 0.0 and np.copysign(1.0, lvls[at]) == 1.0 and cnts[at] == 0
