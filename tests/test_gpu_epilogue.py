"""-m gpu: the Keff epilogue (K5 / K6, xc_finalize.h finalize_body launched by xc_misc.hip launch_finalize) on its own, through
xc_keff_epilogue: per-bin sums, levels, the A(Yeq) table and preY go in straight from the host, so every edge is built exactly,
without a tracer.  Each case is checked against the oracle applied to the same inputs: the sums against its PDF -> CDF tail
(cdf_from_pdf + level_order) bit for bit, the epilogue stage by stage on the kernel's own sums (check_epilogue), and against
the oracle's keff_epilogue of the same sums (check_epilogue_equals).

Which branch of launch_finalize a case takes follows from its thresholds (`branch` below restates them; every case asserts
the branch it is meant to reach): the work arrays take 88 N bytes (2 channels x (pdf + cdf) + 7 epilogue vectors) and move to
global memory past kLdsBudget (150 KiB: N >= 1746); the table joins them in LDS while 88 N + 16 ntbl <= 64 KiB; the workgroup
has 1024 threads when npre > 256, else 512, widened to one thread per sum (2 N, up to 1024) when the reduction is folded in
(LDS work arrays only).  The epilogue runs its two chains per contour in the two halves of the workgroup, so N > half the
workgroup makes threads walk several contours; the cumsum walks N in chunks of 256 with a carry between them."""
import numpy as np
import pytest

import xcontour_oracle as O
from gpu_common import check_epilogue, check_epilogue_equals, same_bits

pytestmark = pytest.mark.gpu

R = O.Rearth
SPHERE = 4 * np.pi * R * R
LDS_BUDGET = 150 * 1024                 # kLdsBudget (xc_internal.h XC_LDS_BUDGET_KB)


def branch(N, ntbl, npre):
    """(work arrays, table, threads per workgroup) that launch_finalize (xc_misc.hip) picks for one xc_keff_epilogue call"""
    lds = 88 * N
    big = lds > LDS_BUDGET
    tbl_lds = not big and lds + 16 * ntbl <= 64 * 1024
    nthr = 1024 if npre > 256 else 512
    if not big:                          # stage 1 folded in: one thread per sum (2 N of them), at most 1024
        nthr = max(nthr, min(1024, (2 * N + 63) // 64 * 64))
    return ('global' if big else 'lds', 'lds' if tbl_lds else 'global', nthr)


def sphere_table(ny, increasing=True, land=()):
    """an A(Yeq) table on ny latitudes, cumulative band areas (rows in `land` hold no area: repeated entries); decreasing = the
    `cdf[-1] - cdf` flip"""
    lat = np.linspace(-90, 90, ny)
    s = np.sin(np.deg2rad(np.r_[-90.0, (lat[1:] + lat[:-1]) / 2, 90.0]))
    rows = 2 * np.pi * R * R * np.diff(s)
    rows[list(land)] = 0.0
    tbl = np.cumsum(np.r_[0.0, rows[:-1]])
    return (tbl if increasing else tbl[-1] - tbl), lat


def levels(N, increase, cd, lo=-1.0, hi=2.0):
    c = np.linspace(lo, hi, N).astype(cd)
    return c if increase else c[::-1].copy()


def area_pdf(rng, N, total=SPHERE):
    """positive per-bin areas summing to about `total` (ascending-value order)"""
    p = rng.random(N) + 0.05
    return p * (total / p.sum())


def run(ctx, pdf, ctr, tbl, crd, increase, lt, cd, pre, mask=1e5, want=None):
    """one slab through xc_keff_epilogue, checked against the oracle on the same inputs; returns (kernel, oracle) dicts"""
    pdf = np.asarray(pdf, dtype=np.float64)
    N = pdf.shape[1]
    if want is not None:
        assert branch(N, len(tbl), 0 if pre is None else len(pre)) == want
    ctr = np.asarray(ctr, dtype=cd)
    out = ctx.keff_epilogue(pdf[None], ctr[None].astype(np.float64), tbl, crd, increase=increase, lt=lt, ctr_dtype=cd,
                            preY=pre, nkeff_mask=mask)
    area, ints = (O.level_order(O.cdf_from_pdf(pdf[c], lt), increase) for c in (0, 1))
    same_bits(out['area'][0], area, 'area')
    same_bits(out['intgrdS'][0], ints, 'intgrdS')
    check_epilogue(out, 0, tbl, crd, pre, cd, mask, ctr=ctr)
    with np.errstate(all='ignore'):
        r = O.keff_epilogue(ctr, area, ints, tbl, crd, pre, mask)
    check_epilogue_equals(out, 0, r)
    return out, r


DIRS = [(inc, lt, cd) for inc in (True, False) for lt in (True, False) for cd in (np.float32, np.float64)]
SIZES = {2: ('lds', 'lds', 512), 3: ('lds', 'lds', 512), 5: ('lds', 'lds', 512),
         255: ('lds', 'lds', 512),       # 255 contours: one short cumsum chunk, the halves of 256 threads cover them
         256: ('lds', 'lds', 512),       # exactly one chunk of 256 (64 lanes x 4)
         257: ('lds', 'lds', 576),       # a second chunk of one element (the carry); 576 threads, halves of 256: two rounds
         513: ('lds', 'lds', 1024),      # three chunks, N % 4 == 1; 1024 threads (the reduction), halves of 512: two rounds
         730: ('lds', 'global', 1024),   # 88 N + 16 x 181 > 64 KiB: the table stays in global memory
         1745: ('lds', 'global', 1024),  # the largest N whose work arrays fit kLdsBudget
         1746: ('global', 'global', 512),    # one more: work arrays in global memory, k_reduce_partials first, 512 threads
         3002: ('global', 'global', 512)}    # thousands of contours, N % 4 == 2, 12 chunks


@pytest.mark.parametrize('N', sorted(SIZES))
@pytest.mark.parametrize('inc,lt,cd', DIRS)
def test_sizes_and_directions(ctx, N, inc, lt, cd):
    rng = np.random.default_rng(N)
    tbl, lat = sphere_table(181)
    pdf = np.stack([area_pdf(rng, N), rng.random(N) * 10.0 ** rng.uniform(-3, 3, N)])
    pre = np.linspace(-89.5, 89.5, 91)
    run(ctx, pdf, levels(N, inc, cd), tbl, lat, inc, lt, cd, pre, want=SIZES[N])


@pytest.mark.parametrize('ntbl,want', [(2, ('lds', 'lds', 512)),
                                       (2990, ('lds', 'lds', 512)),      # 88 x 201 + 16 x 2990 = 65528: just fits beside
                                       (2991, ('lds', 'global', 512)),   # one row more: the table is read from global memory
                                       (5001, ('lds', 'global', 512))])  # longer than the cfg2 table (1801 rows)
@pytest.mark.parametrize('increasing', [True, False])
@pytest.mark.parametrize('lt', [True, False])
def test_table_length_and_placement(ctx, ntbl, want, increasing, lt):
    N = 201
    rng = np.random.default_rng(ntbl)
    tbl, lat = sphere_table(ntbl, increasing)
    pdf = np.stack([area_pdf(rng, N), rng.random(N)])
    pre = np.r_[np.linspace(-90, 90, 77), lat[::max(1, ntbl // 50)]]
    run(ctx, pdf, levels(N, True, np.float32), tbl, lat, True, lt, np.float32, pre, want=want)


@pytest.mark.parametrize('npre', [0, 1, 256, 257, 4000])
@pytest.mark.parametrize('N', [121, 1746])
def test_prey_count(ctx, npre, N):
    """no preY, one, 256 (512 threads), 257 and thousands (1024 threads: launch_finalize widens the workgroup for the
    look-ups) -- on LDS and on global work arrays"""
    rng = np.random.default_rng(npre)
    tbl, lat = sphere_table(181)
    pdf = np.stack([area_pdf(rng, N), rng.random(N)])
    pre = np.sort(rng.uniform(-92, 92, npre))
    big = N > 1745
    want = ('global' if big else 'lds', 'global' if big else 'lds', 1024 if npre > 256 else 512)
    out, _ = run(ctx, pdf, levels(N, True, np.float64), tbl, lat, True, True, np.float64, pre, want=want)
    assert out['interp'].shape == (1, 9, npre)


def _pdf_case(kind, rng, N):
    a, s = area_pdf(rng, N), rng.random(N) * 1e3
    if kind == 'single empty bins':
        a[[3, 10, 11 + 6, N - 5]] = 0.0
    elif kind == 'runs of empty bins':
        a[8:15] = 0.0; a[30:33] = 0.0; s[30:33] = 0.0
    elif kind == 'empty first and last bins':
        a[:2] = 0.0; a[-2:] = 0.0
    elif kind == 'all zero':
        a[:] = 0.0; s[:] = 0.0
    elif kind == 'nan bin':
        a[20] = np.nan; s[40] = np.nan
    elif kind == 'inf bin':
        a[25] = np.inf; s[7] = np.inf; s[50] = -np.inf
    elif kind == 'many decades':
        a *= 10.0 ** rng.uniform(-12, 0, N)
        s = rng.random(N) * 10.0 ** rng.uniform(-150, 150, N)
    return np.stack([a, s])


KINDS = ['single empty bins', 'runs of empty bins', 'empty first and last bins', 'all zero', 'nan bin', 'inf bin', 'many decades']


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('inc,lt,cd', DIRS)
def test_pdf_contents(ctx, kind, inc, lt, cd):
    """empty bins (repeated areas: dA = 0 in the gradient, inf / NaN in dqdA and Leq2, repeated latEq values the look-ups cross),
    a NaN and an infinite sum, sums over hundreds of decades (N = 64, LDS, 512 threads)"""
    N = 64
    rng = np.random.default_rng(KINDS.index(kind))
    tbl, lat = sphere_table(91, inc == lt)
    pdf = _pdf_case(kind, rng, N)
    pre = np.r_[np.linspace(-95, 95, 97), lat[::3]]
    run(ctx, pdf, levels(N, inc, cd), tbl, lat, inc, lt, cd, pre, want=('lds', 'lds', 512))


@pytest.mark.parametrize('increasing', [True, False])
def test_table_with_repeated_rows(ctx, increasing):
    """zero-area land rows repeat table entries: the look-up takes the LAST node of a repeated stretch (np.interp's bracket);
    areas placed exactly on the repeated values and inside the stretches"""
    N = 120
    land = list(range(20, 30)) + [50, 51, 90]
    tbl, lat = sphere_table(121, increasing, land)
    t = np.sort(tbl)
    hit = np.unique(np.r_[t[19:33], t[48:54], t[88:93], t[0], t[-1]])         # areas ON the nodes (repeated ones included)
    area = np.sort(np.r_[hit, np.linspace(t[0], t[-1], N - len(hit))])
    pdf = np.stack([np.r_[area[0], np.diff(area)], np.ones(N)])
    run(ctx, pdf, levels(N, True, np.float64), tbl, lat, True, True, np.float64, np.linspace(-90, 90, 181), want=('lds', 'lds', 512))


@pytest.mark.parametrize('increasing', [True, False])
@pytest.mark.parametrize('lt', [True, False])
def test_lookup_edges(ctx, increasing, lt):
    """an exact table (integer multiples of 2^36: every cumsum exact): areas on table nodes, between them, below the first and one
    ulp above the last; preY outside latEq's range, on latEq's nodes and on a stretch of repeated latEq values (empty bins)"""
    ny, N = 181, 90
    step = 2.0 ** 36
    tbl = np.arange(1, ny + 1) * (4 * step)
    tbl = tbl if increasing else tbl[::-1].copy()
    lat = np.linspace(-90, 90, ny)
    rng = np.random.default_rng(5)
    a = rng.integers(0, 16, N).astype(np.float64) * step                    # whole steps: on nodes when a multiple of 4
    a[10:14] = 0.0                                                          # empty bins: repeated areas, repeated latEq
    a[-1] = np.spacing(4 * step * ny)                                       # the last area one ulp above the table (lt)
    a[-2] = 4 * step * ny - a[:-2].sum() if a[:-2].sum() < 4 * step * ny else 0.0
    s = rng.random(N)
    pdf = np.stack([a, s])
    area = O.cdf_from_pdf(a, lt)
    assert not lt or ((area[:-1] % step == 0).all() and area[-2] == tbl.max() and area[-1] == np.nextafter(tbl.max(), np.inf))
    latEq = O.lookup_coordinates(area, tbl, lat)
    pre = np.r_[-100.0, 100.0, latEq, latEq[11] + 0.0, np.nextafter(latEq[11], -1e3), np.nextafter(latEq[11], 1e3),
                np.linspace(latEq.min(), latEq.max(), 50)]
    run(ctx, pdf, levels(N, True, np.float32), tbl, lat, True, lt, np.float32, pre, want=('lds', 'lds', 512))


@pytest.mark.parametrize('cd', [np.float32, np.float64])
def test_infinite_slopes_and_the_nan_fallback(ctx, cd):
    """three equal levels in a row: dq = 0 there, Leq2 = nkeff = inf.  preY exactly on the latEq node BEFORE an infinite value
    (the bracket's `x == xp[j]` short cut: without it inf * 0 = NaN), inside the bracket after it (slope -inf: inf - inf = NaN,
    numpy's second try from the right node gives inf: interp_eval's NaN fallback) and between two infinite values (the fallback's
    last resort: equal ends)"""
    N = 60
    rng = np.random.default_rng(9)
    tbl, lat = sphere_table(181)
    c = np.linspace(-1.0, 2.0, N)
    c[20:23] = c[21]                                                        # dq[21] = 0
    c[40:44] = c[41]                                                        # dq[41] = dq[42] = 0: two infinite values in a row
    pdf = np.stack([area_pdf(rng, N), rng.random(N) + 0.5])
    area = np.cumsum(pdf[0])
    le = O.lookup_coordinates(area, tbl, lat)
    pre = np.r_[le[19:24], (le[20] + le[21]) / 2, (le[21] + le[22]) / 2, le[40:45], (le[41] + le[42]) / 2,
                (le[42] + le[43]) / 2, np.linspace(-90, 90, 31)]
    out, r = run(ctx, pdf, c.astype(cd), tbl, lat, True, True, cd, pre, want=('lds', 'lds', 512))
    leq = out['Leq2'][0]
    assert np.isinf(leq[[21, 41, 42]]).all() and np.isfinite(leq[20])
    ieq = out['interp'][0, 6]
    assert ieq[1] == leq[20]                                                # on the node before inf: the node's own value
    assert np.isinf(ieq[6]) and np.isinf(ieq[13])                           # after an inf node: the fallback from the right node
    assert np.isinf(ieq[12])                                                # between two infinite values: their common value


@pytest.mark.parametrize('where', ['on', 'ulp below', 'ulp above', 'inf'])
def test_nkeff_mask_cut(ctx, where):
    """nkeff >= mask is NaN (core.py:964): the mask exactly on a value, one ulp either side of it, and at inf (finite values
    pass, infinite ones -- three equal levels -- do not)"""
    N = 50
    rng = np.random.default_rng(17)
    tbl, lat = sphere_table(181)
    c = np.linspace(0.0, 1.0, N); c[30:33] = c[31]
    pdf = np.stack([area_pdf(rng, N), rng.random(N) + 0.5])
    area, ints = np.cumsum(pdf[0]), np.cumsum(pdf[1])
    e = O.keff_epilogue(c, area, ints, tbl, lat, None, np.inf)
    with np.errstate(all='ignore'):
        nk = e['Leq2'] / e['Lmin'] / e['Lmin']                              # unmasked
    idx = int(np.flatnonzero(np.isfinite(nk))[N // 2])
    v = nk[idx]
    mask = {'on': v, 'ulp below': np.nextafter(v, 0.0), 'ulp above': np.nextafter(v, np.inf), 'inf': np.inf}[where]
    out, r = run(ctx, pdf, c, tbl, lat, True, True, np.float64, np.linspace(-90, 90, 19), mask=mask, want=('lds', 'lds', 512))
    got = out['nkeff'][0]
    if out['Lmin'][0][idx] == e['Lmin'][idx]:                               # (else the device cos moved the value by its ulp)
        assert (got[idx] == v) == (where in ('ulp above', 'inf'))
    assert np.isnan(got[31])                                                # inf is never below the mask
    if where == 'inf':
        assert np.isfinite(np.delete(got, 31)).all()
