"""-m gpu: the K8 exact sort (xc_sort.hip) at full size, on its limits and on skewed fields -- exact permutation checks.

Every case (unless it says otherwise) gives the sort the integer payload dA[i] = i + 1: the device's cumulative sum is then
exact and its differences ARE the permutation applied (tests/sort_ref.py); it must equal the oracle's stable argsort, no
tolerance.  Each figure a later change may want (paths, deviations) is printed before it is asserted (pytest -s / -rP).

Which gap each test closes:
  1. what only switches on at size (1801 x 3600 = 6 483 600 cells; 1777 x 3607 = 6 409 639):
       k_range_hist samples one chunk in 16 above 262 144 cells; k_range_bounds folds K1 blocks into groups (per = 2) above
       512 blocks; k_block_exscan carries over 1024-sum rounds above 2.1 M cells (block sums) and over 1024-tile rounds above
       4.2 M cells (tile counts) -- test_full_size_* (all four on every one of them), test_full_size_stack_of_two (per-slab offsets of every
       work array), test_full_size_real_weights_long_double (acum / BPE against a long-double sum)
  2. stability without a tolerance: assert_permutation in every test; test_signed_zeros_keep_their_order
  3. nvalid out of k_fix_runs on block edges: test_nvalid_on_every_edge, test_nvalid_edges_at_full_size
  4. the repair limit FIX_RUN = 128: test_repair_limit
  5. skewed / degenerate value distributions: test_skewed_fields, test_full_size_saturating_profile, test_full_size_bimodal,
     test_strays_one_wave_or_spread, test_strays_both_sides_of_the_T_switch
  6. instantiations: test_float32_mask_instantiations, test_negate_instantiations, test_row_and_slab_payload_in_a_stack
  7. profile and BPE corners: test_profile_exact_Q_and_bpe_tables, test_bpe_masked_plane_through_the_fallback_three_times,
     test_bpe_launch_with_an_all_nan_plane_and_outside_targets
  and test_sort_range_off_in_a_child_takes_path_0 (XC_SORT_RANGE=0: eight passes, the same permutation).

Path assertions: `== 1` only where xc_sort.hip's header promises three passes (ties of any length are never touched; strays in
at most T - 1 K1 groups per side are trimmed wherever they sit; a plateau holding a third of the cells in a thousandth of the
range; runs of at most FIX_RUN cells are repaired) and `== 2` where a run of more than FIX_RUN cells is out of order; elsewhere
`in (1, 2)`, with the reason next to it.  float32 tracers always take path 0.

Cells behind nvalid: include/xcontour_hip.h only says "invalid cells at the end" -- nothing is asserted about their values.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import xcontour_oracle as O
import sort_ref as R
from sort_ref import FIX_C, FIX_RUN, assert_permutation, int_payload
from gpu_common import ROOT, _clean_env

pytestmark = pytest.mark.gpu

NY, NX = 1801, 3600


def run_perm(ctx, q, mask=None, negate=False, order=None, targets=None, what=''):
    """one plane through the sort with the integer payload; exact permutation (and exact Q); returns the path"""
    ny, nx = q.shape
    r = ctx.sort_profile(q, dA=int_payload(ny, nx), mask=mask, targets=targets, want_sorted=True, want_acum=True, negate=negate)
    path = ctx.last_sort_path()
    order, xs = assert_permutation(r, q, mask, negate, order, what=what)
    if targets is not None:
        assert np.array_equal(r['Q'], R.exact_Q(order, xs, targets), equal_nan=True), what + ': Q'
    print('%s: path %d, nvalid %d of %d' % (what, path, r['nvalid'], q.size))
    return path


# ------------------------------------------------------------------------------------------------ full-size fields, made once
class _Fields:
    def __init__(self):
        self.f, self.o = {}, {}

    def field(self, name):
        if name not in self.f:
            self.f[name] = getattr(self, '_' + name)()
        return self.f[name]

    def order(self, name):
        if name not in self.o:
            self.o[name] = R.full_order(self.field(name))
        return self.o[name]

    @staticmethod
    def _grid(ny=NY, nx=NX):
        return np.linspace(0.0, 1.0, ny)[:, None], np.linspace(0.0, 1.0, nx, endpoint=False)[None, :]

    def _pv(self):                       # PV-like: sin(lat) + a wavy jet + noise, 1 % NaN
        rng = np.random.default_rng(101)
        y, x = self._grid()
        phi = (y - 0.5) * np.pi
        q = np.sin(phi) + 0.25 * np.sin(2 * np.pi * 4 * x) * np.cos(phi) ** 2 + 0.02 * rng.standard_normal((NY, NX))
        q[rng.random((NY, NX)) < 0.01] = np.nan
        return q

    def _mask(self):                     # land mask: ~30 % dropped
        return (np.random.default_rng(102).random((NY, NX)) > 0.3).astype(np.float64)

    def _ties(self):
        return np.round(self.field('pv'), 1)

    def _tanh(self):
        """a saturating profile: a tanh front over the lower two thirds of the rows, the upper third on a plateau inside the last
        thousandth of the range (tanh(3.8) = 1 - 1.0e-3 ... tanh(4.4) = 1 - 3.0e-4), wavy in x, plus 1e-9 noise"""
        rng = np.random.default_rng(103)
        y, x = self._grid()
        ye = y + 0.01 * np.sin(2 * np.pi * 5 * x)                       # (not clipped: a clip would pile cells onto one value)
        s = np.where(ye < 2.0 / 3.0, 3.8 * ye * 1.5, 3.8 + 0.6 * (ye - 2.0 / 3.0) * 3.0)
        return np.tanh(s) + 1e-9 * rng.standard_normal((NY, NX))

    def _fill(self):
        rng = np.random.default_rng(104)
        f = rng.standard_normal((NY, NX)) * 10 + 280
        f[17, 33] = 1e20; f[1250, 600] = -9999.0
        return f

    def _bimodal(self):
        rng = np.random.default_rng(105)
        return np.where(rng.random((NY, NX)) < 0.4, -3.0 + 0.01 * rng.standard_normal((NY, NX)), 5.0 + rng.standard_normal((NY, NX)))


@pytest.fixture(scope='module')
def big():
    return _Fields()


# ------------------------------------------------------------------------------------------------------------ A. full size
def test_full_size_pv_field_nan_and_land_mask(ctx, big):
    assert run_perm(ctx, big.field('pv'), big.field('mask'), order=big.order('pv'), what='A pv+mask') == 1


def test_full_size_heavy_ties(ctx, big):
    """~30 distinct values: runs of 10^5 equal keys, the payload order is the stable one (ties are never touched: path 1)"""
    assert run_perm(ctx, big.field('ties'), order=big.order('ties'), what='A ties') == 1


def test_full_size_saturating_profile(ctx, big):
    """the header's own claim: a plateau that holds a third of the cells inside a thousandth of the range keeps its runs short"""
    q = big.field('tanh')
    top = q.max() - 1e-3 * (q.max() - q.min())
    assert 0.30 < (q > top).mean() < 0.40
    assert run_perm(ctx, q, order=big.order('tanh'), what='A tanh plateau') == 1


def test_full_size_fill_value_strays(ctx, big):
    assert run_perm(ctx, big.field('fill'), order=big.order('fill'), what='A fill strays') == 1


def test_full_size_bimodal(ctx, big):
    """two modes of very different width; the equalised key is built for it but the header does not name it: path 1 or 2"""
    assert run_perm(ctx, big.field('bimodal'), order=big.order('bimodal'), what='D bimodal full size') in (1, 2)


def test_full_size_float32(ctx, big):
    """float32 tracers: four passes over the 32-bit key (path 0); 6.48 M floats hold many exact ties"""
    q = big.field('pv').astype(np.float32)
    assert run_perm(ctx, q, big.field('mask'), what='A float32') == 0


@pytest.mark.parametrize('shape', [(NY, NX), (1777, 3607)])
def test_full_size_per_row_payload(ctx, big, shape):
    """XC_DA_ROW: dA[row] = row + 1, the cell's row from a 32-bit divide by nx (3600, and a prime nx where idx / nx is large): the
    sequence of row numbers recovered from acum equals argsort // nx"""
    ny, nx = shape
    if shape == (NY, NX):
        q, order = big.field('pv'), big.order('pv')
    else:
        rng = np.random.default_rng(106)
        y, x = _Fields._grid(ny, nx)
        q = np.cos(3 * y) + 0.1 * np.sin(2 * np.pi * 3 * x) + 0.05 * rng.standard_normal((ny, nx))
        order = R.full_order(q)
    r = ctx.sort_profile(q, dA=np.arange(1, ny + 1, dtype=np.float64), want_sorted=True, want_acum=True)
    m = r['nvalid']
    assert ctx.last_sort_path() == 1 and m == len(order)
    assert np.array_equal(np.diff(r['acum'][:m], prepend=0.0) - 1.0, order // nx)
    assert np.array_equal(r['q_sorted'][:m], q.ravel()[order])


def test_full_size_stack_of_two(ctx, big):
    """two different planes, one shared mask: per-slab offsets of keys, payloads, histograms, block sums at full size"""
    st = np.stack([big.field('pv'), big.field('tanh')])
    mask = big.field('mask')
    r = ctx.sort_profile(st, dA=int_payload(NY, NX), mask=mask, want_sorted=True, want_acum=True)
    assert ctx.last_sort_path() == 1
    for s, name in enumerate(('pv', 'tanh')):
        assert_permutation(r, st[s], mask, order=big.order(name), slab=s, what='A stack slab %d' % s)


def test_full_size_real_weights_long_double(ctx, big):
    """real weights at full size: acum against a LONG-DOUBLE cumulative sum (float64 np.cumsum drifts 7e-14 itself), rel < 1e-12;
    the BPE against the long-double integral, 1e-10; Q through the bracket rule"""
    rng = np.random.default_rng(107)
    q, mask = big.field('pv'), big.field('mask')
    w = rng.random((NY, NX)) + 0.5
    order, xs = R.valid_order(q, mask, order=big.order('pv'))
    ref = R.acum_longdouble(w, order)
    tbl = np.linspace(0.0, float(ref[-1]), 1801)
    cs = np.sin(np.linspace(-1.5, 1.5, 1801))
    tg = np.linspace(0.0, float(ref[-1]), 241)
    r = ctx.sort_profile(q, dA=w, mask=mask, targets=tg, tbl=tbl, coord=cs, want_sorted=True, want_acum=True)
    m = r['nvalid']
    assert ctx.last_sort_path() == 1 and m == len(order) and np.array_equal(r['q_sorted'][:m], xs)
    dev = R.rel_longdouble(r['acum'][:m], ref)
    bref = R.bpe_longdouble(O, xs, w.ravel()[order], tbl, cs)
    bdev = abs(r['bpe'] / bref - 1)
    print('A real weights, %d cells: acum rel %.3e (long double), bpe rel %.3e' % (m, dev, bdev))
    assert dev < 1e-12
    assert bdev < 1e-10
    lo, hi = O.sorted_profile_brackets(ref.astype(np.float64), tg)
    assert all(r['Q'][j] in xs[lo[j]:hi[j] + 1] for j in range(len(tg)))


# ------------------------------------------------------------------------------------------------------------ B. nvalid
def _drop(q, m, rng):
    """exactly q.size - m cells dropped, alternately by NaN and by mask 0"""
    n = q.size
    d = rng.permutation(n)[:n - m]
    q = q.copy()
    mask = np.ones(n)
    q.ravel()[d[0::2]] = np.nan
    mask[d[1::2]] = 0.0
    return q, mask.reshape(q.shape)


NV_N = 5 * 1024
NV_M = (0, 1, 2, 1023, 1024, 1025, 2047, 2048, 2049, NV_N - 1025, NV_N - 1024, NV_N - 1, NV_N)


@pytest.mark.parametrize('kind', ['f64_path1', 'f64_path2', 'f32'])
def test_nvalid_on_every_edge(ctx, kind):
    """the step from the last valid to the first dropped key on, before and behind every edge of k_fix_runs' blocks (FIX_C = 1024
    sorted positions each), block 0 all dropped, the last block none dropped.  path2: distinct values inside 1e-11 between two
    strays (-5, 8.5; K1 does not look at the mask, so they stretch the range dropped or not): the valid cells share one range key
    and go to eight passes as soon as more than FIX_RUN of them are left -- nvalid then comes from k_count_valid."""
    assert R.read_fix_limits() == (FIX_C, FIX_RUN)
    rng = np.random.default_rng(31)
    for m in NV_M:
        if kind == 'f64_path2':
            q0 = 1.0 + 1e-12 * rng.standard_normal((5, 1024))
        else:
            q0 = rng.standard_normal((5, 1024)).astype(np.float32 if kind == 'f32' else np.float64)
        q, mask = _drop(q0, m, rng)
        want = 0 if kind == 'f32' else 1
        if kind == 'f64_path2':
            for cell, v in (((0, 0), -5.0), ((4, 1000), 8.5)):               # a stray on a cell dropped by NaN: dropped by the mask instead
                if np.isnan(q[cell]):
                    mask[cell] = 0.0
                q[cell] = v
            nspike = int(((mask == 1) & ~np.isnan(q) & (np.abs(q - 1.0) < 1e-9)).sum())
            want = 2 if nspike > FIX_RUN else 1
        assert run_perm(ctx, q, mask, what='B %s m=%d' % (kind, m)) == want


def test_nvalid_edges_at_full_size(ctx, big):
    """the same step at full size: n - 1024, n - 1, and the last block edge of k_fix_runs (the largest multiple of FIX_C)"""
    n = NY * NX
    rng = np.random.default_rng(32)
    base, order = big.field('fill'), big.order('fill')                          # no NaN: the count is ours
    for m in (n - 1024, n - 1, n // FIX_C * FIX_C):
        q, mask = _drop(base, m, rng)
        o = order[~np.isnan(q.ravel()[order])]
        assert run_perm(ctx, q, mask, order=o, what='B full size m=n-%d' % (n - m)) == 1


# ------------------------------------------------------------------------------------------------------------ C. repair limit
def _run_plane(off, vals):
    base = np.linspace(0.0, 1.0, 4096 * 8)                                       # spacing 3e-5: far above 2^-23 of the range
    b = base.copy()
    b[off:off + len(vals)] = base[off] + 1e-13 * vals
    # the run is alone in its range key: no other cell within its span (1.3e-11), the neighbours 3e-5 away
    assert (off == 0 or b[off - 1] < b[off:off + len(vals)].min() - 1e-5) and (off + len(vals) == len(b) or b[off + len(vals)] > b[off:off + len(vals)].max() + 1e-5)
    return b.reshape(64, 512)


def test_repair_limit(ctx):
    """runs of 127 / 128 / 129 distinct values 1e-13 apart inside one range key, out of order: FIX_RUN and below are repaired in LDS
    (path 1), one more goes to eight passes (path 2) -- with the run inside a block, its head on the last owned position of a block
    (sorted position % FIX_C == FIX_C - 1: the run then reaches furthest into the window, to FIX_C + FIX_RUN < 1 + FIX_C + 255, so
    a repairable run never touches the window's end) and on the first, straddling two blocks (the right block sees it enter from
    the left: h < 1), at the plane's first and last cells; reversed (every cell moves); 4 values x 32 (ties and inversions)."""
    assert R.read_fix_limits() == (FIX_C, FIX_RUN) == (1024, 128)
    rng = np.random.default_rng(41)
    n = 4096 * 8
    for L in (FIX_RUN - 1, FIX_RUN, FIX_RUN + 1):
        places = {'inside': FIX_C + 300, 'head last owned': 2 * FIX_C - 1, 'head first owned': 2 * FIX_C, 'straddle': 2 * FIX_C - 64,
                  'straddle by one': 3 * FIX_C - L + 1, 'ends on the edge': 3 * FIX_C - L, 'plane start': 0, 'plane end': n - L}
        for name, off in places.items():
            for vals in (rng.permutation(L), np.arange(L)[::-1]):
                path = run_perm(ctx, _run_plane(off, vals.astype(np.float64)), what='C run %d %s' % (L, name))
                assert path == (1 if L <= FIX_RUN else 2), (L, name, path)
    for off in (FIX_C + 300, 2 * FIX_C - 1, 2 * FIX_C - 64):
        vals = rng.permutation(np.repeat(np.arange(4.0), FIX_RUN // 4))
        assert run_perm(ctx, _run_plane(off, vals), what='C 4 x 32 at %d' % off) == 1
        vals = rng.permutation(np.repeat(np.arange(4.0), FIX_RUN // 4 + 1))          # 132 cells: not repaired here
        assert run_perm(ctx, _run_plane(off, vals), what='C 4 x 33 at %d' % off) == 2


# ------------------------------------------------------------------------------------------------------------ D. skewed fields
def _spike(rng, shape):
    return 1.0 + 1e-12 * rng.standard_normal(shape)


def test_skewed_fields(ctx):
    """300 x 700 = 210 000 cells: 52 K1 groups, T = 6 (strays in up to 5 groups per side are trimmed).  Exact in every case."""
    rng = np.random.default_rng(51)
    sh = (300, 700)
    n = sh[0] * sh[1]
    ng, T, first = R.range_groups(n)
    assert (ng, T) == (52, 6)
    one = 1                                         # promised by the header: ties are never touched / few strays are trimmed
    cases = []
    for k in (1, 2, 16, ng):                        # a constant field with strays of distinct, well separated values: only ties
        q = np.full(sh, 2.5)
        q.ravel()[first[np.arange(k) * (ng // k)] + 7] = np.where(np.arange(k) % 2 == 0, -40.0 - np.arange(k), 3.0 + np.arange(k) ** 2)
        cases.append(('constant + %d strays' % k, q, one))
    cases.append(('two plateaus 1e-15 apart', np.where(rng.random(sh) < 0.5, 1.0, 1.0 + 1e-15), one))       # two values: ties only
    cases.append(('two values', rng.integers(0, 2, sh).astype(np.float64), one))
    cases.append(('lognormal', np.exp(3.0 * rng.standard_normal(sh)), None))                 # a heavy tail: not named by the header
    cases.append(('sorted', np.linspace(-1.0, 1.0, n).reshape(sh), None))
    cases.append(('reverse sorted', np.linspace(1.0, -1.0, n).reshape(sh), None))
    cases.append(('denormals', rng.integers(-1000, 1000, sh) * 5e-324, None))                # 256 / width overflows: one key
    q = rng.standard_normal(sh); q[3, 4], q[200, 5] = -1e308, 1e308
    cases.append(('+-1e308 strays (2 groups)', q, one))                                      # trimmed: finite outer widths
    q = rng.standard_normal(sh); q[::7, 3] = -1e308; q[::9, 5] = 1e308
    cases.append(('+-1e308 in 43 / 34 rows', q, None))                                       # more groups than the trim: robust width infinite, one key
    q = rng.standard_normal(sh); q[3, 4], q[5, 6], q[100, 7] = np.inf, -np.inf, np.inf
    cases.append(('+-inf', q, None))                                                         # infinite outer widths collapse
    for name, q, want in cases:
        path = run_perm(ctx, q, what='D ' + name)
        assert path == want if want else path in (1, 2), (name, path)


def test_signed_zeros_keep_their_order(ctx):
    """+0.0 and -0.0 are one value (the key folds -0.0 onto +0.0, as numpy's stable sort compares them equal): a third of the cells
    each, interleaved, the rest noise -- the zeros come out in their original order, with three passes (ties are never touched)"""
    rng = np.random.default_rng(52)
    sh = (300, 700)
    u = rng.random(sh)
    q = np.where(u < 1 / 3, 0.0, np.where(u < 2 / 3, -0.0, rng.standard_normal(sh)))
    assert np.signbit(q).any() and (q == 0).sum() > 100000
    assert run_perm(ctx, q, what='D signed zeros') == 1
    assert run_perm(ctx, q, negate=True, what='D signed zeros negated') == 1
    assert run_perm(ctx, q.astype(np.float32), what='D signed zeros float32') == 0


@pytest.mark.parametrize('count,one_wave,want', [(3, True, 1), (3, False, 1), (8, True, 1), (8, False, 1), (9, True, None), (9, False, None)])
def test_strays_one_wave_or_spread(ctx, count, one_wave, want):
    """600 x 700: 103 K1 groups, T = 9.  Distinct values inside 1e-11 (any stretch of the robust range sends them to one key) and
    strays below AND above in `count` groups that all fall to wave 0 of k_range_bounds (g % 8 == 0: it names only its two
    smallest / largest) or are dealt over the eight waves.  The header: up to eight stray-holding groups are trimmed wherever they
    sit -- path 1; nine: in one wave they still are, spread they reach the 9th candidate -- not promised either way."""
    rng = np.random.default_rng(53)
    sh = (600, 700)
    ng, T, _ = R.range_groups(sh[0] * sh[1])
    assert (ng, T) == (103, 9)
    q = _spike(rng, sh)
    c = R.stray_cells(q.size, count, one_wave)
    q.ravel()[c] = -5.0 - np.arange(count)
    q.ravel()[c + 11] = 8.5 + 2.0 * np.arange(count)
    path = run_perm(ctx, q, what='D %d stray groups, %s' % (count, 'one wave' if one_wave else 'spread'))
    assert path == want if want else path in (1, 2)


@pytest.mark.parametrize('ng_want,count,want', [(7, 1, None), (8, 1, None), (16, 1, 1), (71, 7, 1), (71, 8, None), (72, 8, 1)])
def test_strays_both_sides_of_the_T_switch(ctx, ng_want, count, want):
    """T = 9 from 72 groups, ng / 8 below, 1 below 16 (the exact extrema): strays in T - 1 groups per side are trimmed (path 1),
    in T groups they bound the robust range (the spike collapses into one key: expected 2, not promised)"""
    rng = np.random.default_rng(54)
    sh = (ng_want * 8, 512)
    ng, T, _ = R.range_groups(sh[0] * sh[1])
    assert ng == ng_want and T == (9 if ng >= 72 else max(ng // 8, 1))
    assert (count <= T - 1) == (want == 1)
    q = _spike(rng, sh)
    c = R.stray_cells(q.size, count, False)
    q.ravel()[c] = -5.0 - np.arange(count)
    q.ravel()[c + 11] = 8.5 + 2.0 * np.arange(count)
    path = run_perm(ctx, q, what='D ng=%d T=%d, %d stray groups' % (ng, T, count))
    assert path == want if want else path in (1, 2)


# ------------------------------------------------------------------------------------------------------------ E. instantiations
def _stack_field(rng, S, ny, nx, dt):
    q = np.round(rng.standard_normal((S, ny, nx)) * 3, 2).astype(dt)                        # ties, negatives, zeros
    q[rng.random(q.shape) < 0.02] = np.nan
    return q


@pytest.mark.parametrize('dt', [np.float64, np.float32])
@pytest.mark.parametrize('per_slab', [False, True])
def test_float32_mask_instantiations(ctx, dt, per_slab):
    """a float32 mask selects k_radix_hist / k_radix_scatter<K, true, TQ, float, ...> and k_range_hist<TQ, float>"""
    rng = np.random.default_rng(61)
    S, ny, nx = 3, 193, 170
    q = _stack_field(rng, S, ny, nx, dt)
    mask = (rng.random((S, ny, nx) if per_slab else (ny, nx)) > 0.3).astype(np.float32)
    mask[..., 5, :] = 0.5                                                                   # only 1 is valid
    r = ctx.sort_profile(q, dA=int_payload(ny, nx), mask=mask, want_sorted=True, want_acum=True)
    assert ctx.last_sort_path() == (1 if dt == np.float64 else 0)
    for s in range(S):
        assert_permutation(r, q[s], mask[s] if per_slab else mask, slab=s, what='E f32 mask slab %d' % s)
    if not per_slab:                                                                        # and a single plane
        run_perm(ctx, q[0], mask, what='E f32 mask single plane')


def test_negate_instantiations(ctx):
    """negate: float32; float64 with asymmetric strays (range_params swaps and negates all four bounds, the outer zones differ:
    one far stray below, three near ones above, 4 groups <= T - 1 = 5: path 1); +-inf; a 3-plane stack with an all-NaN plane"""
    rng = np.random.default_rng(62)
    sh = (300, 700)
    assert run_perm(ctx, rng.standard_normal(sh).astype(np.float32), negate=True, what='E negate float32') == 0
    q = _spike(rng, sh)
    _, _, first = R.range_groups(q.size)
    q.ravel()[first[3] + 9] = -1e6
    q.ravel()[first[[10, 20, 30]] + 9] = (7.0, 8.0, 9.5)
    assert run_perm(ctx, q, negate=True, what='E negate asymmetric strays') == 1
    assert run_perm(ctx, q, negate=False, what='E asymmetric strays') == 1
    qi = rng.standard_normal(sh); qi[3, 4], qi[5, 6], qi[100, 7] = np.inf, -np.inf, np.inf
    mask = (rng.random(sh) > 0.3).astype(np.float64)
    assert run_perm(ctx, qi, mask, negate=True, what='E negate +-inf') in (1, 2)             # infinite outer widths: not promised
    S, ny, nx = 3, 193, 170
    st = _stack_field(rng, S, ny, nx, np.float64)
    st[1] = np.nan
    r = ctx.sort_profile(st, dA=int_payload(ny, nx), want_sorted=True, want_acum=True, negate=True)
    assert ctx.last_sort_path() == 1 and r['nvalid'][1] == 0
    for s in range(S):
        assert_permutation(r, st[s], negate=True, slab=s, what='E negate stack slab %d' % s)


def test_row_and_slab_payload_in_a_stack(ctx):
    """XC_DA_ROW in a stack (rows recovered per plane) and XC_DA_SLAB with negate (every plane's payload names its plane)"""
    rng = np.random.default_rng(63)
    S, ny, nx = 3, 211, 173
    n = ny * nx
    q = _stack_field(rng, S, ny, nx, np.float64)
    r = ctx.sort_profile(q, dA=np.arange(1, ny + 1, dtype=np.float64), want_sorted=True, want_acum=True)
    assert ctx.last_sort_path() == 1
    for s in range(S):
        order, xs = R.valid_order(q[s])
        m = int(r['nvalid'][s])
        assert m == len(order) and np.array_equal(r['q_sorted'][s][:m], xs)
        assert np.array_equal(np.diff(r['acum'][s][:m], prepend=0.0) - 1.0, order // nx)
    for dt in (np.float64, np.float32):
        dA = np.stack([int_payload(ny, nx, s) for s in range(S)])
        qq = q.astype(dt)
        r = ctx.sort_profile(qq, dA=dA, want_sorted=True, want_acum=True, negate=True)
        for s in range(S):
            assert_permutation(r, qq[s], negate=True, slab=s, payload_slab=s, what='E slab payload negate slab %d' % s)


# ------------------------------------------------------------------------------------------------------------ F. profile, BPE
def _table(total, ntbl, increasing):
    tbl = np.linspace(0.0, total, ntbl)
    cs = np.sin(np.linspace(-1.2, 1.4, ntbl)) * 50.0
    return (tbl, cs) if increasing else (tbl[::-1].copy(), cs[::-1].copy())


@pytest.mark.parametrize('J', [1, 256, 257, 1000])
def test_profile_exact_Q_and_bpe_tables(ctx, J):
    """J targets through k_profile (no table: 1, 1, 2, 4 workgroups) and riding in k_bpe (nprof 1, 1, 2, 4), integer payload: Q equals
    the 'right' rule for EVERY target -- half-integers, targets equal to an acum value, below acum[0], above acum[-1]; the BPE of
    increasing and decreasing tables of 2, 2048 (LDS), 2049 and 5000 (global bracket search) entries against the oracle"""
    rng = np.random.default_rng(64 + J)
    ny, nx = 97, 339                                                                        # 32 883 cells: ragged last tile
    q = np.round(rng.standard_normal((ny, nx)), 2)
    q[rng.random((ny, nx)) < 0.02] = np.nan
    mask = (rng.random((ny, nx)) > 0.2).astype(np.float64)
    dA = int_payload(ny, nx)
    order, xs = R.valid_order(q, mask)
    tg = R.targets_for(order, J, rng)
    want = R.exact_Q(order, xs, tg)
    r = ctx.sort_profile(q, dA=dA, mask=mask, targets=tg, want_sorted=True, want_acum=True)
    assert_permutation(r, q, mask, what='F J=%d' % J)
    assert np.array_equal(r['Q'], want)
    total = float(np.sum(order + 1.0))
    for ntbl in (2, 2048, 2049, 5000):
        for inc in (True, False):
            tbl, cs = _table(total * 0.9, ntbl, inc)                                        # (cells beyond the table's end too)
            r = ctx.sort_profile(q, dA=dA, mask=mask, targets=tg, tbl=tbl, coord=cs)
            assert np.array_equal(r['Q'], want), (ntbl, inc)
            ref = O.bpe_integral(q, dA, tbl, cs, mask)
            assert abs(r['bpe'] / ref - 1) < 1e-10, (ntbl, inc, r['bpe'], ref)


def test_bpe_masked_plane_through_the_fallback_three_times(ctx):
    """a plane with dropped cells that fails the range-key check: the tail (scan, profile, BPE) runs twice with nvalid < n, the
    arrival ticket of k_bpe is re-armed each time -- three calls in a row on one context, the oracle's value every time"""
    rng = np.random.default_rng(65)
    ny, nx = 64, 512
    q0 = _spike(rng, (ny, nx)); q0[::7, 3] = -5.0; q0[::9, 5] = 8.5
    q, mask = _drop(q0, ny * nx - 5000, rng)
    dA = rng.random((ny, nx)) + 0.5
    order, xs = R.valid_order(q, mask)
    ws = dA.ravel()[order]
    tbl, cs = _table(float(ws.sum()), 300, False)
    tg = np.linspace(-1.0, ws.sum() * 1.1, 300)
    ref = O.bpe_integral(q, dA, tbl, cs, mask)
    Qo, _, acum = O.sorted_profile(q, dA, tg, mask)
    lo, hi = O.sorted_profile_brackets(acum, tg)
    for rep in range(3):
        r = ctx.sort_profile(q, dA=dA, mask=mask, targets=tg, tbl=tbl, coord=cs, want_sorted=True, want_acum=True)
        assert ctx.last_sort_path() == 2 and r['nvalid'] == len(order) == ny * nx - 5000
        assert np.array_equal(r['q_sorted'][:len(xs)], xs)
        dev = R.rel_longdouble(r['acum'][:len(xs)], R.acum_longdouble(dA, order))
        print('F fallback, %d cells: acum rel %.3e (long double), bpe rel %.3e' % (len(xs), dev, abs(r['bpe'] / ref - 1)))
        assert dev < 1e-12
        assert abs(r['bpe'] / ref - 1) < 1e-10, rep
        assert all(r['Q'][j] in xs[lo[j]:hi[j] + 1] for j in range(len(tg)))
    run_perm(ctx, q, mask, what='F fallback plane, integer payload')


def test_bpe_launch_with_an_all_nan_plane_and_outside_targets(ctx):
    """k_bpe with nprof = 2 on a stack whose middle plane has no valid cell: NaN for every target there and a BPE of 0 (the oracle's
    empty sum); targets below acum[0] and above acum[-1] on the others"""
    rng = np.random.default_rng(66)
    S, ny, nx = 3, 61, 130
    q = _stack_field(rng, S, ny, nx, np.float64)
    q[1] = np.nan
    dA = int_payload(ny, nx)
    tg = np.concatenate(([-5.0, 0.0, 0.5], np.floor(rng.random(294) * ny * nx * (ny * nx + 1) / 2) + 0.5, [1e18, 3e13, 4e13]))
    tbl, cs = _table(ny * nx * (ny * nx + 1) / 2.0, 181, True)
    r = ctx.sort_profile(q, dA=dA, targets=tg, tbl=tbl, coord=cs, want_sorted=True, want_acum=True)
    assert list(r['nvalid'] > 0) == [True, False, True]
    for s in range(S):
        order, xs = assert_permutation(r, q[s], slab=s, what='F NaN plane stack slab %d' % s)
        assert np.array_equal(r['Q'][s], R.exact_Q(order, xs, tg), equal_nan=True)
        assert r['bpe'][s] == 0.0 if s == 1 else abs(r['bpe'][s] / O.bpe_integral(q[s], dA, tbl, cs) - 1) < 1e-10


# ------------------------------------------------------------------------------------------------------------ G. knob
def test_sort_range_off_in_a_child_takes_path_0(ctx, tmp_path):
    """XC_SORT_RANGE=0 (read when a context is made): float64 tracers take the eight key passes (path 0) and give the permutation
    the three-pass path gives here -- a fresh child process, its results in a file"""
    out = str(tmp_path / 'child.json')
    env = _clean_env()
    env['XC_SORT_RANGE'] = '0'
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'sort_ref.py'), out], env=env, cwd=ROOT, timeout=300,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert p.returncode == 0, p.stderr[-3000:]
    with open(out) as f:
        res = json.load(f)
    for name, (q, mask) in R.child_cases().items():
        order, _ = R.valid_order(q, mask)
        assert res[name]['path'] == 0 and res[name]['nvalid'] == len(order)
        assert np.array_equal(np.asarray(res[name]['perm'], dtype=np.int64), order), name
        assert run_perm(ctx, q, mask, what='G ' + name + ' in this process') == 1
    assert len(R.valid_order(*R.child_cases()['nvalid_1025'])[0]) == 1025
