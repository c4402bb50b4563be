"""-m gpu: K9 box-counting crossing (xc_cross.hip k_crossing + k_crossing_reduce) where its launch geometry changes: level counts on
both sides of every switch of the launcher and of the kernel's epilogue, more tiles than blocks, and the output forms without
counts / without lengths.  Every case is a small plane against the oracle.

Main bar: areas whose square roots are small integers, so every box weight sqrt(area) * stride is an integer and every partial
sum, in any order (the +w / -w difference array, its prefix and suffix scans, the per-block partials, the reduction), stays far
below 2^53: the oracle's lengths are exact and the kernel's must equal them bit for bit -- np.array_equal, no tolerance.

The geometry a test claims to reach is asserted on `crossing_geometry`, a test-side restatement of the launcher's arithmetic, not
on a record from the library (there is none for K9)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import xcontour_oracle as O
from test_gpu_parity import rel
from gpu_common import ROOT, _clean_env

pytestmark = pytest.mark.gpu

LDS_BUDGET = 150 * 1024                  # kLdsBudget (xc_internal.h XC_LDS_BUDGET_KB)
CROSS_RB, CROSS_TPB, CROSS_W1 = 32, 256, 252


def crossing_geometry(N, nslab, ny, nx, pad_x, stride, full_width, blocks=2048):
    """(ncopy, lds_bytes, two, ntj, nti, bps) of one xc_crossing call: a restatement of xc_cross.hip launch_crossing -- the lines
    that set `np`, `ncopy`, `lds`, `coarse`, `nbj` / `nbi`, `cols` / `nbw` / `rbox` / `tw`, `ntj` / `nti` and `bps` (`blocks` is the
    XC_CROSS_BLOCKS knob, 2048 when unset) -- and of the kernel epilogue's `two = (N - (N + 1) / 2 + 63) / 64 <= 8` (prefix and
    suffix scan, or prefix only).  The two must be edited together.

    A test asserts on this that its OWN parameters give the geometry it claims (4 copies, more tiles than blocks, ...): that catches
    a test whose parameters have drifted.  It does NOT catch a launcher that has drifted away from this restatement: the library
    keeps no record of a K9 launch to compare with.

    lds_bytes above LDS_BUDGET is the call the launcher refuses ("too many contours for one pass")."""
    np_ = (N + 1) | 1
    ncopy = 8
    while ncopy > 1 and (2 * N + 3) * 8 + ncopy * np_ * 12 > 48 * 1024:
        ncopy >>= 1
    lds = (2 * N + 3) * 8 + ncopy * np_ * 12
    coarse = lambda n: int(np.round(n / stride))                    # round half to even of the true quotient
    Jn, In = coarse(ny), coarse(nx + pad_x)
    nbj, nbi = Jn - 1, (In if full_width else min(Jn, In)) - 1
    assert nbj >= 1 and nbi >= 1 and nbj * stride <= ny - 1 and nbi * stride <= nx + pad_x - 1
    cols = 6 <= stride <= 63
    nbw = 63 // stride if cols else 0
    rbox = max(64 // stride, 1) if cols else CROSS_RB
    tw = CROSS_W1 if stride == 1 else CROSS_TPB
    ntj = (nbj + rbox - 1) // rbox
    nti = ((nbi + nbw - 1) // nbw + 3) // 4 if cols else (nbi + tw - 1) // tw
    bps = min(max(blocks // nslab, 8), ntj * nti)
    two = (N - (N + 1) // 2 + 63) // 64 <= 8
    return ncopy, lds, two, ntj, nti, bps


def compaction_chunks(N):
    """rounds of the kernel's copies -> compact loop `for (k0 = 0; k0 <= N; k0 += CROSS_TPB)`"""
    return N // CROSS_TPB + 1


# ---------------------------------------------------------------- inputs
def exact_area(ny, nx, dt, j0):
    """areas whose square roots are the integers 1..5 (exact in float32 and float64, and so is every sum of sqrt(area) * stride);
    a NaN, a negative and a +inf area at the coarse boxes (j0, 3), (j0 + 1, 1), (j0 + 2, 2): np.nansum skips the first two, the third
    makes every level its box crosses +inf (the kernel's direct sums `s_dir`)"""
    j, i = np.arange(ny)[:, None], np.arange(nx)[None, :]
    a = ((1 + (7 * j + 3 * i) % 5) ** 2).astype(dt)
    a[j0, 3] = np.nan; a[j0 + 1, 1] = -4.0; a[j0 + 2, 2] = np.inf
    return a


def fraction_field(rng, nslab, ny, nx, noise=0.04):
    """a gradient 0 .. 1 along y plus noise, cut to [0, 1]: an interior box spans ~0.1 of the range"""
    return np.clip(np.linspace(0.0, 1.0, ny)[None, :, None] + noise * rng.standard_normal((nslab, ny, nx)), 0.0, 1.0)


def field_on_levels(rng, F, lev, L0, L1, dt, specials=True):
    """the tracer of a case: F mapped onto the middle 10/12 of [L0, L1] (levels spread over [L0, L1] reach 10 % beyond the field
    on both sides), then ~10 % of the cells set exactly ON a level of their slab (for float32: on the level rounded to float32),
    5 % one ulp above and 5 % one ulp below -- as test_crossing_values_on_and_next_to_levels does -- a few NaN cells, a band of
    all-NaN rows in slab 1, a +inf cell in slab 0 and a -inf cell in the last slab.  `lev`: (N,) or (nslab, N)."""
    nslab, ny, nx = F.shape
    lo, hi = L0 + (L1 - L0) / 12.0, L1 - (L1 - L0) / 12.0
    q = (lo + (hi - lo) * F).astype(dt)
    levs = np.broadcast_to(np.asarray(lev, dtype=np.float64), (nslab, np.shape(lev)[-1]))
    for s in range(nslab):
        inside = np.flatnonzero((levs[s] >= lo) & (levs[s] <= hi))
        if inside.size == 0:
            continue
        v = levs[s][rng.choice(inside, size=(ny, nx))].astype(dt)
        on = rng.random((ny, nx))
        q[s] = np.where(on < 0.10, v, q[s])
        q[s] = np.where((on >= 0.10) & (on < 0.15), np.nextafter(v, dt(np.inf)), q[s])
        q[s] = np.where((on >= 0.15) & (on < 0.20), np.nextafter(v, dt(-np.inf)), q[s])
    if specials:
        q[0, 5, 7] = np.nan; q[0, ny // 3, nx // 2] = np.nan; q[nslab - 1, ny - 3, nx - 2] = np.nan
        if nslab > 1:
            q[1, ny // 3:ny // 3 + 5, :] = np.nan
        q[0, ny // 4, nx - 5] = np.inf
        q[nslab - 1, 3 * ny // 4, 4] = -np.inf
    assert q.dtype == dt
    return q


def level_sets(rng, N, nslab):
    """the level sets of one N as (name, levels, L0, L1): equally spaced; the same with a jitter of +-0.004 of a spacing (still
    equally spaced to the kernel's 0.01 test, with a wide verification zone); sorted uniform random levels with one duplicated
    pair, one set PER SLAB (the scan route); float32 contours of a 300 +- 1 field (equally spaced to the kernel only while N is
    small: from about N = 1000 on the float32 rounding exceeds 0.01 of a spacing and the scan route takes over)"""
    lin = np.linspace(-1.2, 1.2, N)
    jit = lin + rng.uniform(-0.004, 0.004, N) * (2.4 / max(N - 1, 1))
    assert (np.diff(jit) > 0).all()
    rnd = np.sort(rng.uniform(-1.2, 1.2, (nslab, N)), axis=1)
    if N > 4:
        rnd[:, N // 3] = rnd[:, N // 3 + 1]                        # a duplicated pair
    f32 = np.linspace(299.0, 301.0, N).astype(np.float32).astype(np.float64)
    return [('linspace', lin, -1.2, 1.2), ('jitter', jit, -1.2, 1.2), ('random', rnd, -1.2, 1.2), ('f32-300', f32, 299.0, 301.0)]


def oracle_of(q, lev, area, stride, pad, mode, full):
    """[(lengths, counts)] of every slab from the oracle on the padded slab"""
    ap = O.pad_x(area, pad, mode)
    lev = np.asarray(lev)
    return [O.contour_crossing(O.pad_x(q[s], pad, mode), lev[s] if lev.ndim == 2 else lev, ap, stride, full) for s in range(q.shape[0])]


def check_exact(ctx, q, lev, area, stride, pad, mode, full, what):
    """counts and lengths of every slab bit for bit the oracle's (exact-weight areas); returns the oracle's results"""
    lens, cnts = ctx.crossing(q, lev, area, stride=stride, pad_x=pad, pad_mode=mode, full_width=full)
    ref = oracle_of(q, lev, area, stride, pad, mode, full)
    for s, (ol, oc) in enumerate(ref):
        assert np.array_equal(cnts[s].astype(np.int64), oc), (what, s, 'counts')
        assert np.array_equal(lens[s], ol), (what, s, 'lengths', float(np.nanmax(np.abs(np.where(np.isfinite(ol), lens[s] - ol, 0.0)))))
    return ref


# ---------------------------------------------------------------- 0. the restatement itself
# (N, compaction chunks, LDS copies, prefix + suffix epilogue, dynamic LDS above 64 KB)
SWITCHES = [(201, 1, 8, True, False),
            (255, 1, 8, True, False), (256, 2, 8, True, False),
            (436, 2, 8, True, False), (437, 2, 4, True, False),
            (766, 3, 4, True, False), (767, 3, 2, True, False),
            (1025, 5, 2, True, False), (1026, 5, 2, False, False),
            (1227, 5, 2, False, False), (1228, 5, 1, False, False),
            (2338, 10, 1, False, False), (2339, 10, 1, False, True),
            (5484, 22, 1, False, True)]
NY2, NX2, NSLAB2 = 64, 300, 3             # section 2's plane: 63 x 300 = 18 900 boxes, 2 x 2 tiles


def test_switches_of_the_restatement():
    """every switch sits where the table of SWITCHES says: the first N on the other side differs from the last N on this side in
    exactly the quantity the pair is there for, and 5485 levels are over the LDS budget"""
    geo = {N: crossing_geometry(N, NSLAB2, NY2, NX2, 1, 1, True) for N in range(1, 5487)}
    first = lambda pred: next(N for N in range(1, 5487) if pred(N))
    assert first(lambda N: compaction_chunks(N) == 2) == 256
    assert first(lambda N: geo[N][0] == 4) == 437
    assert first(lambda N: geo[N][0] == 2) == 767
    assert first(lambda N: not geo[N][2]) == 1026
    assert first(lambda N: geo[N][0] == 1) == 1228
    assert first(lambda N: geo[N][1] > 64 * 1024) == 2339
    assert first(lambda N: geo[N][1] > LDS_BUDGET) == 5485
    for N, chunks, ncopy, two, attr in SWITCHES:
        assert (compaction_chunks(N), geo[N][0], geo[N][2], geo[N][1] > 64 * 1024) == (chunks, ncopy, two, attr), N
        assert geo[N][3:] == (2, 2, 4) and geo[N][1] <= LDS_BUDGET


# ---------------------------------------------------------------- 2. level counts on both sides of every switch
@pytest.mark.parametrize('N,chunks,ncopy,two,attr', SWITCHES)
def test_crossing_level_counts_on_both_sides_of_every_switch(ctx, N, chunks, ncopy, two, attr):
    """N levels on a 64 x 300 plane (stride 1, one wrapped column, full width, 3 slabs, 2 x 2 tiles), float32 and float64 tracer, the
    four level sets of `level_sets`, exact-weight areas: counts and lengths bit for bit the oracle's.  N runs over both sides of
    1 -> 2 compaction chunks (255 | 256), 8 -> 4 -> 2 -> 1 LDS copies (436 | 437, 766 | 767, 1227 | 1228), prefix + suffix -> prefix
    only (1025 | 1026), dynamic LDS beyond 64 KB (2338 | 2339) and the largest N the LDS budget takes (5484); 201 is the N DESIGN.md
    quotes timings at.  The levels the field does not reach (10 % at either end) are exact zeros; the NaN, negative and +inf areas
    sit in crossed boxes."""
    g = crossing_geometry(N, NSLAB2, NY2, NX2, 1, 1, True)
    assert (compaction_chunks(N), g[0], g[2], g[1] > 64 * 1024) == (chunks, ncopy, two, attr) and g[1] <= LDS_BUDGET
    assert g[3:] == (2, 2, 4)                                         # 2 x 2 tiles, one block each
    rng = np.random.default_rng(9000 + N)
    F = fraction_field(rng, NSLAB2, NY2, NX2)
    j0 = NY2 // 2
    for dt in (np.float64, np.float32):
        area = exact_area(NY2, NX2, dt, j0)
        for name, lev, L0, L1 in level_sets(rng, N, NSLAB2):
            q = field_on_levels(rng, F, lev, L0, L1, dt)
            what = (N, np.dtype(dt).name, name)
            ref = check_exact(ctx, q, lev, area, 1, 1, 'wrap', True, what)
            # the inputs do what the case is there for
            mn, mx = O._box_minmax(O.pad_x(q[0], 1, 'wrap'), 1, NY2 - 1, NX2)
            l0 = lev[0] if np.ndim(lev) == 2 else lev
            for (j, i) in ((j0, 3), (j0 + 1, 1), (j0 + 2, 2)):
                assert ((l0 >= mn[j, i]) & (l0 < mx[j, i])).any(), (what, 'special area not in a crossed box', j, i)
            assert all(np.isinf(ol).any() for ol, _ in ref), what
            if name != 'random':
                # +inf in slab 0 crosses every level above it, -inf in slab 2 every level below it; slab 1 has neither
                assert ref[1][1][0] == 0 and ref[1][1][-1] == 0 and ref[0][1][0] == 0 and ref[2][1][-1] == 0, what
                assert ref[1][1].max() > 0
            if name == 'linspace':
                per_box = np.searchsorted(l0, mx[20:44], 'left') - np.searchsorted(l0, mn[20:44], 'left')
                assert np.median(per_box) >= 0.04 * N, what               # interior boxes cross tens of levels (10 at N = 255)


def test_crossing_refuses_more_levels_than_the_lds_budget_takes(ctx):
    """N = 5485 is one level more than fits 150 KB of LDS with one copy: the launcher's own error, and the context works afterwards"""
    from xcontour_amd._native import XContourHipError
    assert crossing_geometry(5484, 1, 20, 40, 1, 1, True)[1] <= LDS_BUDGET < crossing_geometry(5485, 1, 20, 40, 1, 1, True)[1]
    rng = np.random.default_rng(5485)
    F = fraction_field(rng, 1, 20, 40)
    area = exact_area(20, 40, np.float64, 8)
    lev = np.linspace(-1.2, 1.2, 5485)
    q = field_on_levels(rng, F, lev, -1.2, 1.2, np.float64)
    with pytest.raises(XContourHipError, match='xc_crossing: too many contours for one pass'):
        ctx.crossing(q, lev, area, stride=1, pad_x=1, pad_mode='wrap', full_width=True)
    lev = np.linspace(-1.2, 1.2, 17)
    check_exact(ctx, field_on_levels(rng, F, lev, -1.2, 1.2, np.float64), lev, area, 1, 1, 'wrap', True, 'N = 17 after the refusal')


# the largest |error| / bound seen by the test below, per N (printed; the bound itself comes from the oracle alone)
RATIO_SEEN = {}


@pytest.mark.parametrize('N', [201, 1025, 1026, 2339])
def test_crossing_level_counts_with_rounded_weights(ctx, N):
    """random float64 areas (weights that round) on section 2's plane, equally spaced levels, both tracer dtypes.  Counts exact.
    N <= 1025 (prefix + suffix epilogue): the project's bar for K9 lengths, rel < 1e-13.  N > 1025 (prefix only): a level's sum is a
    prefix over ALL lower difference cells, so its rounding error scales with the whole mass of the slab, not with the level; the
    bar is the standard forward bound of a floating-point sum, |lens - oracle| <= n 2^-53 W per level, with W the sum of the finite
    box weights of the slab (the oracle's own `w`) and n the number of additions that can enter one level: two per crossed box
    (+w and -w), N for the prefix, bps block partials, 256 for the reduction.  The largest error / bound is printed."""
    g = crossing_geometry(N, NSLAB2, NY2, NX2, 1, 1, True)
    assert g[2] == (N <= 1025) and g[3:] == (2, 2, 4)
    bps = g[5]
    rng = np.random.default_rng(7000 + N)
    F = fraction_field(rng, NSLAB2, NY2, NX2)
    area = rng.random((NY2, NX2)) * 9 + 1
    area[NY2 // 2, 3] = np.nan; area[NY2 // 2 + 1, 1] = -1.0
    lev = np.linspace(-1.2, 1.2, N)
    ap = O.pad_x(area, 1, 'wrap')
    nbj, nbi = NY2 - 1, NX2
    with np.errstate(invalid='ignore'):
        w = np.sqrt(ap[:nbj, :nbi]).astype(np.float64) * 1                  # the oracle's `w` (contour_crossing)
    worst = 0.0
    for dt in (np.float64, np.float32):
        q = field_on_levels(rng, F, lev, -1.2, 1.2, dt)
        lens, cnts = ctx.crossing(q, lev, area, stride=1, pad_x=1, pad_mode='wrap', full_width=True)
        for s, (ol, oc) in enumerate(oracle_of(q, lev, area, 1, 1, 'wrap', True)):
            assert np.array_equal(cnts[s].astype(np.int64), oc), (N, s)
            assert np.isfinite(ol).all() and np.isfinite(lens[s]).all()
            if N <= 1025:
                assert rel(lens[s], ol) < 1e-13, (N, s, rel(lens[s], ol))
                continue
            mn, mx = O._box_minmax(O.pad_x(q[s], 1, 'wrap'), 1, nbj, nbi)
            crossed = np.searchsorted(lev, mx, 'left') > np.searchsorted(lev, mn, 'left')       # some level in [mn, mx); NaN sorts last on both sides
            n = 2 * int(np.count_nonzero(crossed)) + N + bps + 256
            bound = n * 2.0 ** -53 * float(w[np.isfinite(w)].sum())
            err = float(np.abs(lens[s] - ol).max())
            worst = max(worst, err / bound)
            print('K9 rounded weights N = %d %s slab %d: max |err| %.3e, bound %.3e, ratio %.3e' % (N, np.dtype(dt).name, s, err, bound, err / bound))
            assert err <= bound, (N, s, err, bound)
            assert (lens[s][oc == 0] == 0.0).all()
    RATIO_SEEN[N] = worst


# ---------------------------------------------------------------- 3. more tiles than blocks
def test_crossing_stack_of_256_slabs_two_tiles_per_block(ctx):
    """the stacked call the kernel is mapped for: 256 float32 slabs of 140 x 600 (four distinct planes repeated), so bps = 8 blocks
    per slab own 5 x 3 = 15 tiles -- seven blocks walk two tiles, one block one.  Exact-weight area shared by all slabs, 33 equally
    spaced levels: every one of the 256 outputs is bit for bit the oracle's result of its distinct plane."""
    ny, nx, S, N = 140, 600, 256, 33
    ncopy, lds, two, ntj, nti, bps = crossing_geometry(N, S, ny, nx, 1, 1, True)
    assert (ntj, nti) == (5, 3) and bps == 8 < ntj * nti and ncopy == 8 and two
    rng = np.random.default_rng(256)
    lev = np.linspace(-1.2, 1.2, N)
    base = field_on_levels(rng, fraction_field(rng, 4, ny, nx), lev, -1.2, 1.2, np.float32)
    area = exact_area(ny, nx, np.float32, ny // 2)
    ref = oracle_of(base, lev, area, 1, 1, 'wrap', True)
    assert len(set(r[0].tobytes() for r in ref)) == 4                      # four distinct answers
    idx = np.arange(S) % 4
    lens, cnts = ctx.crossing(base[idx], lev, area, stride=1, pad_x=1, pad_mode='wrap', full_width=True)
    for s in range(S):
        ol, oc = ref[idx[s]]
        assert np.array_equal(cnts[s].astype(np.int64), oc), s
        assert np.array_equal(lens[s], ol), s


# (stride, ny, nx, pad, mode, full_width): each has more than 8 tiles and no multiple of 8 (the last round of the tile loop is ragged)
FEW_BLOCKS_CASES = [(1, 140, 600, 1, 'wrap', True),              # S = 1: 5 x 3 tiles
                    (2, 300, 620, 2, 'wrap', True),              # S = 2: 5 x 2
                    (4, 520, 1040, 4, 'edge', True),             # S = 4: 5 x 2
                    (3, 400, 790, 3, 'reflect', True),           # S = 0 (run-time stride): 5 x 2
                    (7, 300, 301, 7, 'symmetric', True),         # S = -1 (lanes along fine columns): 5 x 2, 9 x 9 boxes per wave
                    (16, 330, 400, 16, 'wrap', True),            # S = -1: 5 x 3 tiles of 4 x 12 boxes
                    (1, 300, 600, 1, 'edge', False),             # not full width: nbi = min(Jn, In) - 1 = 299 box columns, 10 x 2
                    (1, 170, 255, 3, 'constant', True)]          # NaN-filled padding: columns 255..257 lie in the SECOND tile column, 6 x 2


def run_more_tiles_than_blocks(ctx):
    """the body of test_crossing_more_tiles_than_blocks, run in its child process (XC_CROSS_BLOCKS=8)"""
    assert os.environ.get('XC_CROSS_BLOCKS') == '8'
    nslab = 3
    for stride, ny, nx, pad, mode, full in FEW_BLOCKS_CASES:
        rng = np.random.default_rng(100 * stride + ny)
        F = fraction_field(rng, nslab, ny, nx)
        j0 = (int(np.round(ny / stride)) - 1) // 2
        for N, want_copies in ((33, 8), (500, 4)):
            ncopy, lds, two, ntj, nti, bps = crossing_geometry(N, nslab, ny, nx, pad, stride, full, blocks=8)
            assert ncopy == want_copies and bps == 8 < ntj * nti and (ntj * nti) % bps != 0, (stride, ny, nx, ntj, nti, bps)
            if mode == 'constant':
                assert nx + pad - 1 > CROSS_W1 and nx > CROSS_W1           # padded corner columns are served by the second tile column
            lin = np.linspace(-1.2, 1.2, N)
            rnd = np.sort(rng.uniform(-1.2, 1.2, N)); rnd[N // 3] = rnd[N // 3 + 1]
            for dt in (np.float64, np.float32):
                area = exact_area(ny, nx, dt, j0)
                for name, lev in (('linspace', lin), ('random', rnd)):
                    q = field_on_levels(rng, F, lev, -1.2, 1.2, dt)
                    ref = check_exact(ctx, q, lev, area, stride, pad, mode, full, (stride, ny, nx, mode, full, N, np.dtype(dt).name, name))
                    assert all(oc.max() > 0 for _, oc in ref)


def test_crossing_more_tiles_than_blocks():
    """XC_CROSS_BLOCKS=8 in a child process (the knob is read when the context is created): 3 slabs share 8 blocks per slab over 10,
    12, 15 or 20 tiles, so the tile loop runs a second and a ragged third round -- its per-wave `continue`, the carried guess of the
    scan route, partial sums that live across tiles.  Every stride class of the kernel (1, 2, 4, run-time 3, lanes along the fine
    columns for 7 and 16), a call that is not full width and one whose NaN-filled padding lies in a second tile column; 33 levels
    (8 copies) and 500 (4 copies), equally spaced and random, both tracer dtypes, exact-weight areas: bit for bit the oracle."""
    env = _clean_env()
    env['XC_CROSS_BLOCKS'] = '8'
    src = 'import sys; sys.path[:0] = [%r, %r, %r]\n' % (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')) \
        + 'import test_gpu_crossing_geometry as T\nfrom xcontour_amd import _native as nat\nctx = nat.Context(0)\n' \
        + 'T.run_more_tiles_than_blocks(ctx)\nctx.close()\nprint("OK")\n'
    p = subprocess.run([sys.executable, '-c', src], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert p.returncode == 0 and 'OK' in p.stdout, p.stdout[-3000:]


# ---------------------------------------------------------------- 4. lengths without counts, counts without lengths
def crossing_one_output(ctx, q, lev, area, stride, pad, mode, full, want):
    """xc_crossing through ctypes with out_cnt == NULL (want = 'len': the CNT = false kernels) or out_len == NULL (want = 'cnt':
    k_crossing_reduce without lengths); Context.crossing always asks for both"""
    from xcontour_amd import _native as nat
    q, lev, area = np.ascontiguousarray(q), np.ascontiguousarray(lev, dtype=np.float64), np.ascontiguousarray(area)
    nslab, ny, nx = q.shape
    N = lev.shape[-1]
    out = np.full((nslab, N), -7.0) if want == 'len' else np.full((nslab, N), 2 ** 64 - 7, dtype=np.uint64)    # (values no result has)
    ctx._check(ctx.lib.xc_crossing(ctx.handle, q.ctypes.data, nat.dtype_code(q.dtype), nslab, ny, nx, pad, nat.PAD_MODES[mode],
                                   lev.ctypes.data, N, 1 if lev.ndim == 2 else 0, area.ctypes.data, nat.dtype_code(area.dtype),
                                   1 if area.ndim == 3 else 0, stride, 1 if full else 0,
                                   out.ctypes.data if want == 'len' else None, out.ctypes.data if want == 'cnt' else None))
    return out


ONE_OUT_NY, ONE_OUT_NX = 70, 330


@pytest.mark.parametrize('stride', [1, 2, 4, 3, 7])
def test_crossing_lengths_without_counts_and_counts_without_lengths(ctx, stride):
    """out_cnt == NULL launches k_crossing<TQ, TA, false, S>: per stride class both tracer and both area dtypes, i.e. all 20 such
    instantiations over the five strides; N = 33 and N = 1026 (prefix-only epilogue, 2 copies), equally spaced and random levels.
    With exact-weight areas every term is an integer, so no cancellation residue exists and the lengths equal the oracle's bit for
    bit even without the counts' exact-zero rule.  out_len == NULL must give the oracle's counts."""
    ny, nx, nslab, pad = ONE_OUT_NY, ONE_OUT_NX, 2, stride
    rng = np.random.default_rng(40 + stride)
    F = fraction_field(rng, nslab, ny, nx)
    j0 = (int(np.round(ny / stride)) - 1) // 2
    for N in (33, 1026):
        g = crossing_geometry(N, nslab, ny, nx, pad, stride, True)
        assert g[2] == (N == 33) and g[0] == (8 if N == 33 else 2)
        lin = np.linspace(-1.2, 1.2, N)
        rnd = np.sort(rng.uniform(-1.2, 1.2, N)); rnd[N // 3] = rnd[N // 3 + 1]
        for name, lev in (('linspace', lin), ('random', rnd)):
            for qdt in (np.float64, np.float32):
                q = field_on_levels(rng, F, lev, -1.2, 1.2, qdt)
                ref = oracle_of(q, lev, exact_area(ny, nx, np.float64, j0), stride, pad, 'wrap', True)
                assert all(oc.max() > 0 and oc.min() == 0 for _, oc in ref[1:])
                for adt in (np.float64, np.float32):
                    area = exact_area(ny, nx, adt, j0)                     # the same integer weights in either dtype
                    what = (stride, N, name, np.dtype(qdt).name, np.dtype(adt).name)
                    lens = crossing_one_output(ctx, q, lev, area, stride, pad, 'wrap', True, 'len')
                    cnts = crossing_one_output(ctx, q, lev, area, stride, pad, 'wrap', True, 'cnt')
                    for s, (ol, oc) in enumerate(ref):
                        assert np.array_equal(lens[s], ol), (what, s)
                        assert np.array_equal(cnts[s].astype(np.int64), oc), (what, s)


def test_crossing_lengths_without_counts_rounded_weights(ctx):
    """random float64 areas, equally spaced levels, out_cnt == NULL: crossed levels at the project's bar for K9 lengths
    (rel < 1e-13).  Levels that no box crosses are NOT required to be exact zeros here: without the counts the kernel cannot tell
    such a level from one whose differences cancel, and its comment promises agreement to ~1e-15 of the largest level; asserted
    as |lens| <= 1e-13 * max(oracle) on the uncrossed levels."""
    ny, nx, nslab, N = ONE_OUT_NY, ONE_OUT_NX, 2, 33
    rng = np.random.default_rng(4)
    F = fraction_field(rng, nslab, ny, nx)
    area = rng.random((ny, nx)) * 9 + 1
    area[ny // 2, 3] = np.nan; area[ny // 2 + 1, 1] = -1.0
    lev = np.linspace(-1.2, 1.2, N)
    for stride in (1, 7):
        for qdt in (np.float64, np.float32):
            q = field_on_levels(rng, F, lev, -1.2, 1.2, qdt, specials=False)
            lens = crossing_one_output(ctx, q, lev, area, stride, stride, 'wrap', True, 'len')
            for s, (ol, oc) in enumerate(oracle_of(q, lev, area, stride, stride, 'wrap', True)):
                crossed = oc > 0
                assert crossed.any() and not crossed.all() and np.isfinite(ol).all()
                assert rel(lens[s][crossed], ol[crossed]) < 1e-13, (stride, s)
                assert (np.abs(lens[s][~crossed]) <= 1e-13 * ol.max()).all(), (stride, s)
