"""Every instantiation of the histogram pass -- K3 (k_hist, xc_hist_kernel.h; its deterministic twin in xc_hist_det.hip) and K3S
(k_keff_single, xc_keff1.hip) -- reached through the public paths, on weights that vary along x, checked bin by bin against an exact
(math.fsum) reference of the weights the kernel forms.

Why x-varying weights: `cell_area(lat, lon)` is constant along a row, so a kernel that takes the weight of the wrong column inside its
row (two cells of a lane swapped, a wrong offset in a ragged last strip) passes every test that uses it.  Here
dA[j, i] = cell_area[j] (1 + 0.25 f(j, i)) with a hashed f that differs in every column and every row.

Each row of VARIANTS names the instantiation it must reach and the smallest input that reaches it; the test asserts the record of
xc_last_hist_variant (Context.last_hist_variant) and the sums.  test_every_instantiation_has_a_row lists the kernels of the gfx950
code object of the built library and fails on one that has no row here."""
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import xcontour_oracle as O
from gpu_common import ROOT, bits, _clean_env

U = 2.0 ** -53
TESTS = os.path.dirname(os.path.abspath(__file__))


# ------------------------------------------------------------------------------------------------------------------- inputs
def hashed(ny, nx, salt=0):
    """f(j, i) in [-1, 1): a different value in every column and every row"""
    j = np.arange(ny, dtype=np.uint64)[:, None]; i = np.arange(nx, dtype=np.uint64)[None, :]
    h = (j * np.uint64(2654435761) + i * np.uint64(40503) + np.uint64(salt) * np.uint64(97)) * np.uint64(2246822519)
    h = (h ^ (h >> np.uint64(13))) & np.uint64(0xffffffff)
    return h.astype(np.float64) / 2.0 ** 31 - 1.0


def grid(ny, nx):
    lat = np.linspace(-88.0, 88.0, ny)
    lon = np.arange(nx) * (360.0 / nx)
    return lat, lon


def xvar_dA(ny, nx, kind='plane', nslab=1, salt=0):
    """x-varying, strictly positive, finite weights ('plane', 'slab'), the same with zeros for land ('land': FAST stays on), with one
    NaN ('nan': FAST goes off); 'row' one value per row, 'none' no weights"""
    lat, lon = grid(ny, nx)
    base = O.cell_area(lat, lon) * (1.0 + 0.25 * hashed(ny, nx, salt))
    if kind == 'none':
        return None
    if kind == 'row':
        return np.ascontiguousarray(base[:, 0] * (1.0 + 0.01 * np.arange(ny)))
    if kind == 'land':
        base[2:5, 3:nx // 3] = 0.0
        base[:, nx - 1] = 0.0
    if kind == 'nan':
        base[ny // 2, nx - 2] = np.nan
    if kind == 'slab':
        return np.stack([base * (1.0 + 0.125 * hashed(ny, nx, salt + 1 + s)) for s in range(nslab)])
    return base


def tracer(nslab, ny, nx, dt, seed, nan=True):
    rng = np.random.default_rng(seed)
    lat, lon = grid(ny, nx)
    la, lo = np.deg2rad(lat)[:, None], np.deg2rad(lon)[None, :]
    q = np.stack([np.sin(la * (1 + s)) + 0.3 * np.cos(3 * lo + s) * np.cos(la) + 0.05 * rng.standard_normal((ny, nx))
                  for s in range(nslab)]).astype(dt)
    if nan and ny > 4:
        q[:, ny // 3, :] = np.nan                                  # a whole NaN row
        q[:, rng.integers(1, ny - 1, 5), rng.integers(0, nx, 5)] = np.nan
    return q


def poke_levels(q, values, seed):
    """cells exactly on a level and one ulp to either side (in the tracer dtype), away from the extrema"""
    rng = np.random.default_rng(seed)
    dt = q.dtype.type
    S, ny, nx = q.shape
    for s in range(S):
        vs = np.asarray(values[s] if np.ndim(values) == 2 else values)
        for k in rng.choice(np.arange(1, len(vs) - 1), min(6, len(vs) - 2), replace=False):
            v = dt(vs[k])
            for t in (v, np.nextafter(v, dt(np.inf)), np.nextafter(v, dt(-np.inf))):
                q[s, rng.integers(1, ny - 1) if ny > 2 else 0, rng.integers(0, nx)] = t
    return q


# ------------------------------------------------------------------------------------------------------------------- reference
def grad2(q, rdx, rdy, periodic):
    """the squared gradient in the kernel's order of operations (oracle.grad2_sphere when periodic; one-sided, spacing dx, at walls)"""
    q = np.asarray(q, dtype=np.float64)
    ny = q.shape[0]
    if periodic:
        gx = (np.roll(q, -1, axis=1) - np.roll(q, 1, axis=1)) * rdx[:, None]
    else:
        E = np.concatenate([q[:, 1:], q[:, -1:]], axis=1); W = np.concatenate([q[:, :1], q[:, :-1]], axis=1)
        gx = (E - W) * rdx[:, None]
        gx[:, 0] *= 2.0; gx[:, -1] *= 2.0
    jn = np.minimum(np.arange(ny) + 1, ny - 1); js = np.maximum(np.arange(ny) - 1, 0)
    gy = (q[jn, :] - q[js, :]) * rdy[:, None]
    return gx * gx + gy * gy


def nan0(w):
    return np.where(np.isnan(w), 0.0, w)


def bin_index(x, edges, closed):
    """np.digitize convention (weighted_histogram): 1..nb in range, anything else dropped; closed: the last edge belongs to bin nb"""
    x = np.asarray(x, dtype=np.float64).ravel()
    nb = len(edges) - 1
    idx = np.digitize(x, edges)
    if closed:
        idx = np.where(x == edges[-1], nb, idx)
    return idx


class Exact(object):
    """exact per-bin and prefix sums (math.fsum) of one slab's weights, with the sums of |w| that bound their rounding"""

    def __init__(self, idx, w, nb):
        w = np.asarray(w, dtype=np.float64).ravel()
        ok = (idx >= 1) & (idx <= nb)
        b, v = idx[ok] - 1, w[ok]
        order = np.argsort(b, kind='stable')
        b, v = b[order], v[order]
        self.ends = np.searchsorted(b, np.arange(nb), side='right')
        starts = np.concatenate([[0], self.ends[:-1]])
        vl = v.tolist()
        self.pdf = np.array([math.fsum(vl[a:e]) for a, e in zip(starts, self.ends)])
        self.n = self.ends - starts
        self.absb = np.array([math.fsum(np.abs(v[a:e]).tolist()) for a, e in zip(starts, self.ends)])
        self.prefix = np.array([math.fsum(vl[:e]) for e in self.ends])
        self.total = math.fsum(vl)
        self.abs_total = math.fsum(np.abs(v).tolist())
        self.nb = nb

    def check_pdf(self, got, what, extra=0.0):
        """|gpu - exact| <= (n_bin + 2) 2^-53 sum_bin |w| (any order of float64 additions), + extra sum_bin |w|"""
        err = np.abs(np.asarray(got) - self.pdf)
        bound = (self.n + 2) * U * self.absb + extra * self.absb
        bad = ~(err <= bound)
        if bad.any():
            k = int(np.flatnonzero(bad)[0])
            raise AssertionError('%s: bin %d of %d: gpu %r, exact %r, bound %.3g (%d bins fail)' % (what, k, self.nb, float(got[k]),
                                 float(self.pdf[k]), bound[k], int(bad.sum())))

    def check_cdf(self, got_asc, lt, what, extra=0.0):
        """entries of the cumulative sums (ascending-value order) against the exact prefix: each bounded by the cells and bins that
        enter it; the flipped form (lt=False: cdf[-1] - cdf) by the total"""
        got_asc = np.asarray(got_asc)
        k = np.arange(self.nb)
        cabs = np.cumsum(self.absb)
        if lt:
            exact = self.prefix
            bound = (self.ends + 3 * (k + 1) + 2) * U * cabs + extra * cabs
        else:
            exact = np.array([math.fsum([self.total, -p]) for p in self.prefix])
            bound = 2 * (self.ends[-1] + 3 * self.nb + 2) * U * self.abs_total + extra * self.abs_total
        err = np.abs(got_asc - exact)
        bad = ~(err <= bound)
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            raise AssertionError('%s: entry %d of %d (lt=%s): gpu %r, exact %r, bound %.3g (%d entries fail)'
                                 % (what, i, self.nb, lt, float(got_asc[i]), float(exact[i]), bound[i], int(bad.sum())))


# ------------------------------------------------------------------------------------------------------------------- the table
# key: (kernel, q dtype, VEC, NINT, GRAD, DA2D, NEXT, FAST, DET, E32) for k_hist, (kernel, q dtype, DA2D, FAST, WCNT) for K3S
def k3_keys():
    keys = []
    for dt in ('f64', 'f32'):
        for vec in (1, 2):
            for det in (0, 3):
                kern = 'K3' if det == 0 else 'K3-det'
                for nint in (0, 1, 2):
                    for grad in (False, True):
                        for da2d in (False, True):
                            keys.append((kern, dt, vec, nint, grad, da2d, False, False, det, False))
                            if (nint == 0 and grad) or (nint == 1 and not grad):
                                keys.append((kern, dt, vec, nint, grad, da2d, True, False, det, False))
                for nxt in (False, True):
                    if vec == 2 and det == 0:
                        for da2d in (False, True):
                            keys.append((kern, dt, 2, 0, True, da2d, nxt, True, 0, False))
                    if vec == 2 and det == 3:
                        keys.append((kern, dt, 2, 0, True, True, nxt, True, 3, False))
        for nxt in (False, True):
            keys.append(('K3', dt, 4, 0, True, True, nxt, True, 0, False))
    for nxt in (False, True):
        keys.append(('K3', 'f32', 4, 0, True, True, nxt, True, 0, True))               # E32
        keys.append(('K3', 'f32', 4, 1, False, True, nxt, False, 0, False))            # supplied float32 grdS
    return keys


def k3s_keys():
    return [('K3S', dt, da2d, fast, wcnt) for dt in ('f64', 'f32') for da2d in (False, True) for fast in (False, True)
            for wcnt in (False, True)]


DT = {'f64': np.float64, 'f32': np.float32}


def row_for(key):
    """the smallest input that reaches instantiation `key` through a public path"""
    if key[0] == 'K3S':
        _, dt, da2d, fast, wcnt = key
        return dict(path='plan', dt=dt, ny=128, nx=512, N=37, da=('plane' if da2d else 'row'), periodic=None if fast else False,
                    counts=wcnt, single=True)
    kern, dt, vec, nint, grad, da2d, nxt, fast, det, e32 = key
    detb = det == 3
    if vec == 4:
        r = dict(path='plan', dt=dt, ny=12, nx=1024 + 16, N=29, da='plane', chain=nxt, ctr='f32' if e32 else 'f64', nslab=2)
        if nint == 1:
            r.update(supplied='f32', ctr='f32')
        if dt == 'f64':
            r['env'] = {'XC_HIST_VEC4': '1'}
        return r
    nx = 130 if vec == 2 else 131
    keff = nxt or (fast and da2d)                    # q_next rides in xc_keff_dev only; FAST + plane dA: dA_pos_finite comes from KeffPlan
    if keff:
        r = dict(path='plan', dt=dt, ny=20, nx=nx, N=23, nslab=2, chain=nxt, det=detb)
        if nint == 1:
            r.update(supplied='f64', da='plane' if da2d else 'row')
        elif fast:
            r.update(da='land' if da2d else 'row')
        else:
            r.update(da='nan' if da2d else 'row', periodic=False if not da2d else None)
        return r
    # Context.hist: never FAST with weights (it does not vouch for them): FAST = no dA, the in-kernel gradient, half-open last bin
    r = dict(path='hist', dt=dt, ny=18, nx=nx, nslab=2, nint=nint, grad=grad, det=detb, nb=19, last_closed=not fast)
    r['da'] = ('none' if (fast or (not grad and nint == 0)) else 'row') if not da2d else ('slab' if nint == 2 else 'plane')
    if fast:
        r['da'] = 'none'
    return r


ALL_KEYS = k3_keys() + k3s_keys()
# rows reached a second way: a NaN in dA / the numpy last bin also take FAST off (K3S), two slabs under single_read='force',
# the float32 four-cell variant without E32 through N = 2049 and through XC_HIST_E32=0, XC_HIST_VEC4=0
EXTRA = [
    (('K3S', 'f64', True, False, True), dict(path='plan', dt='f64', ny=128, nx=512, N=37, da='nan', counts=True, single=True)),
    (('K3S', 'f32', True, False, False), dict(path='plan', dt='f32', ny=128, nx=512, N=37, da='plane', right_edge='numpy',
                                             counts=False, single=True)),
    # float32 levels over a range of ~54 ulps: NOT equally spaced to a quarter of a bin, K3S takes its general search (rows re-read)
    (('K3S', 'f32', True, True, True), dict(path='plan', dt='f32', ny=128, nx=512, N=37, da='plane', counts=True, single=True, tiny=True)),
    (('K3', 'f32', 4, 0, True, True, False, True, 0, False), dict(path='plan', dt='f32', ny=12, nx=1024, N=2049, da='plane', ctr='f32',
                                                                 nslab=2)),
    (('K3', 'f32', 4, 0, True, True, True, True, 0, False), dict(path='plan', dt='f32', ny=12, nx=1024, N=29, da='plane', ctr='f32',
                                                                nslab=2, chain=True, env={'XC_HIST_E32': '0'})),
    (('K3', 'f32', 2, 0, True, True, False, True, 0, False), dict(path='plan', dt='f32', ny=12, nx=1024, N=29, da='land', ctr='f32',
                                                                 nslab=2, env={'XC_HIST_VEC4': '0'})),
]
ROWS = [(k, row_for(k)) for k in ALL_KEYS] + EXTRA
for k, r in list(ROWS):
    if k[0] == 'K3S':
        ROWS.append((k, dict(r, nslab=2, force=True)))


def expected(key):
    if key[0] == 'K3S':
        _, dt, da2d, fast, wcnt = key
        return dict(kernel='K3S', q_dtype=np.dtype(DT[dt]), vec=2, nint=0, grad=1, da2d=int(da2d), next=0, fast=int(fast), e32=0,
                    det=0, wcnt=int(wcnt))
    kern, dt, vec, nint, grad, da2d, nxt, fast, det, e32 = key
    return dict(kernel=kern, q_dtype=np.dtype(DT[dt]), vec=vec, nint=nint, grad=int(grad), da2d=int(da2d), next=int(nxt),
                fast=int(fast), e32=int(e32), det=det, wcnt=0)


def row_id(kr):
    k, r = kr
    s = '-'.join(str(int(x)) if isinstance(x, bool) else str(x) for x in k)
    return s + ('-force2' if r.get('force') else '') + ('-' + '_'.join('%s%s' % kv for kv in sorted(r.get('env', {}).items())) if r.get('env') else '') \
        + ('-N%d' % r['N'] if r.get('N') == 2049 else '') + ('-%s' % r['da'] if r.get('da') in ('nan',) and k[0] == 'K3S' else '') \
        + ('-numpy' if r.get('right_edge') == 'numpy' else '') + ('-tiny' if r.get('tiny') else '')


# ------------------------------------------------------------------------------------------------------------------- runners
def run_hist(ctx, r, seed=0):
    dt = DT[r['dt']]
    S, ny, nx, nb = r.get('nslab', 2), r['ny'], r['nx'], r['nb']
    q = tracer(S, ny, nx, dt, seed)
    edges = np.linspace(-1.1, 1.1, nb + 1)
    q = poke_levels(q, edges, seed)
    q[0, ny // 2, nx // 2] = dt(edges[-1])                                       # on the last edge: the last-bin rule decides
    lat, lon = grid(ny, nx)
    dA = xvar_dA(ny, nx, r['da'], S, seed)
    rng = np.random.default_rng(seed + 7)
    integ = [(rng.random((S, ny, nx)) * 3.0 + 0.1), rng.standard_normal((S, ny, nx)) * 10.0 ** rng.integers(-3, 3, (S, ny, nx))][:r['nint']]
    prod_f32 = r.get('prod_f32', False)
    grad = None
    if r['grad']:
        rdx, rdy = O.grad_metrics(lat, lon)
        grad = (rdx, rdy, r.get('periodic', True))
    out = ctx.hist(q, edges, dA, integ, grad=grad, last_closed=r['last_closed'], lt=r.get('lt', True), prod_f32=prod_f32,
                   deterministic=r['det'])
    v = ctx.last_hist_variant()
    for s in r.get('check_slabs', range(S)):
        d = np.ones((ny, nx)) if dA is None else (dA[s] if dA.ndim == 3 else (dA[:, None] * np.ones((1, nx)) if dA.ndim == 1 else dA))
        w = [nan0(d)]
        for g in integ:
            p = (g[s].astype(np.float32) * d.astype(np.float32)).astype(np.float64) if prod_f32 else g[s] * d
            w.append(nan0(p))
        if grad is not None:
            w.append(nan0(grad2(q[s], grad[0], grad[1], grad[2]) * d))
        idx = bin_index(q[s], edges, r['last_closed'])
        cnt = np.bincount(idx, minlength=nb + 2)[1:nb + 1]
        assert np.array_equal(out['counts'][s].astype(np.int64), cnt), 'counts, slab %d' % s
        for ch, wc in enumerate(w):
            ex = Exact(idx, wc, nb)
            ex.check_pdf(out['pdf'][s, ch], 'pdf slab %d channel %d' % (s, ch), extra=2.0 ** -48 if r['det'] else 0.0)
            c = np.cumsum(out['pdf'][s, ch])
            if not r.get('lt', True):
                c = c[-1] - c
            assert np.array_equal(bits(out['cdf'][s, ch]), bits(c)), 'cdf is not the sequential cumsum of the pdf'
            ex.check_cdf(out['cdf'][s, ch], r.get('lt', True), 'cdf slab %d channel %d' % (s, ch), extra=2.0 ** -48 if r['det'] else 0.0)
            if r['det'] and r['last_closed'] and not (grad is not None and ch == len(w) - 1):
                # the fixed-point rule bit for bit: the window from the bound the library takes before the pass
                dmax = 1.0 if dA is None else float(np.abs(dA[np.isfinite(dA)]).max())
                bound = dmax if ch == 0 else float(np.abs(integ[ch - 1][s]).max()) * dmax
                od, _ = O.weighted_histogram(q[s].astype(np.float64), edges, wc, 'numpy', deterministic=True,
                                             det_top=O.det_window_top(bound))
                assert np.array_equal(bits(out['pdf'][s, ch]), bits(od)), 'deterministic sums, slab %d channel %d' % (s, ch)
    return v


def make_plan(ctx, r, q, dA, lat, lon, **kw):
    from xcontour_amd.pipeline import KeffPlan
    ny = r['ny']
    tbl = np.cumsum(O.cell_area(lat, lon).sum(axis=1))
    single = ('force' if r.get('force') else True) if r.get('single') else False
    p = KeffPlan(ctx, q.shape[0], ny, r['nx'], r['N'], DT[r['dt']], DT[r.get('ctr', r['dt'])], dA=dA, lat=lat, lon=lon,
                 tbl=tbl, tbl_coord=lat, periodic_x=r.get('periodic') is not False, increase=r.get('increase', True),
                 lt=r.get('lt', True), right_edge=r.get('right_edge', 'xhistogram'), grdS_dtype=DT.get(r.get('supplied')),
                 deterministic=r.get('det', False), counts=r.get('counts', True), single_read=single, **kw)
    p.set_q(q)
    return p


def run_plan(ctx, r, seed=0, with_chain_twin=True):
    dt = DT[r['dt']]
    S, ny, nx, N = r.get('nslab', 1), r['ny'], r['nx'], r['N']
    cdt = DT[r.get('ctr', r['dt'])]
    inc, lt = r.get('increase', True), r.get('lt', True)
    re_ = r.get('right_edge', 'xhistogram')
    lat, lon = grid(ny, nx)
    q = tracer(S, ny, nx, dt, seed)
    if r.get('tiny'):
        q = (300.0 + 54 * 2.0 ** -15 * (q.astype(np.float64) - np.nanmin(q)) / (np.nanmax(q) - np.nanmin(q))).astype(dt)
    ctr = np.stack([O.cal_contours(q[s], N, inc, cdt) for s in range(S)])
    q = poke_levels(q, ctr, seed)
    dA = xvar_dA(ny, nx, r['da'], S, seed)
    g = None
    if r.get('supplied'):
        g = (np.random.default_rng(seed + 3).random((S, ny, nx)) * 2.0 + 0.01).astype(DT[r['supplied']])
        g[:, 4, 5] = -0.5                                              # a signed integrand
    p = make_plan(ctx, r, q, dA, lat, lon)
    if g is not None:
        p.set_grdS(g)
    p.run(chain=r.get('chain', False))
    v = ctx.last_hist_variant()
    out = p.fetch()
    assert p.replays == 0
    rdx, rdy = O.grad_metrics(lat, lon)
    periodic = r.get('periodic') is not False
    for s in range(S):
        assert np.array_equal(out['ctr'][s], ctr[s].astype(np.float64)), 'levels, slab %d' % s
        edges, binc = O.hist_edges(ctr[s])
        if re_ == 'xhistogram':
            edges = np.concatenate((edges[:-1], edges[-1:] + 1e-8))
        edges = edges.astype(np.float64)
        d = np.ones((ny, nx)) if dA is None else (dA[s] if dA.ndim == 3 else (dA[:, None] * np.ones((1, nx)) if dA.ndim == 1 else dA))
        w0 = nan0(d)
        w1 = nan0((g[s].astype(np.float64) if g is not None else grad2(q[s], rdx, rdy, periodic)) * d)
        idx = bin_index(q[s], edges, re_ == 'numpy')
        cnt = np.bincount(idx, minlength=N + 2)[1:N + 1]
        if r.get('counts', True):
            assert np.array_equal(out['counts'][s].astype(np.int64), O.level_order(cnt, binc)), 'counts, slab %d' % s
        for name, w in (('area', w0), ('intgrdS', w1)):
            ex = Exact(idx, w, N)
            got = O.level_order(out[name][s], binc)                   # back to ascending-value order
            ex.check_cdf(got, lt, '%s slab %d' % (name, s), extra=2.0 ** -48 if r.get('det') else 0.0)
    return v, out


# ------------------------------------------------------------------------------------------------------------------- tests
def check_variant(v, key, r):
    want = expected(key)
    got = {k: v[k] for k in want}
    assert got == want, 'reached %r, wanted %r' % (got, want)
    if key[0] == 'K3S':
        assert v['G'] >= 8 and v['G'] % 8 == 0 and v['cps'] >= 1 and 4 <= v['rpc'] and v['nstrip'] >= 1
    else:
        assert v['threads'] in (512, 1024) and v['bps'] >= 1 and v['ncopy'] >= 1
        assert v['nstrip'] == -(-r['nx'] // (64 * key[2]))


def run_row(ctx, key, r):
    if r['path'] == 'hist':
        v = run_hist(ctx, r)
    else:
        v, out = run_plan(ctx, r)
        if key[0] == 'K3S':
            # against the chain on the same inputs: levels, counts and status bit for bit, the sums within the same per-entry bound
            rc = dict(r, single=False, force=False)
            vc, oc = run_plan(ctx, rc)
            assert vc['kernel'] == 'K3'
            for k in ('ctr', 'status') + (('counts',) if r.get('counts', True) else ()):
                assert np.array_equal(out[k], oc[k]), k
    check_variant(v, key, r)
    return v


def child(code, env_extra, timeout=600):
    env = _clean_env()
    env.update(env_extra)
    src = 'import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)\n' % (ROOT, os.path.join(ROOT, 'oracle'), TESTS) \
        + 'import test_gpu_hist_variants as T\nfrom xcontour_amd import _native as nat\nctx = nat.Context(0)\n' + code + '\nprint("OK")\n'
    p = subprocess.run([sys.executable, '-c', src], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True, timeout=timeout)
    assert p.returncode == 0 and 'OK' in p.stdout, p.stdout[-3000:]
    return p.stdout


@pytest.mark.gpu
@pytest.mark.parametrize('kr', ROWS, ids=[row_id(x) for x in ROWS])
def test_variant(ctx, kr):
    key, r = kr
    if r.get('env'):
        child('T.run_row(ctx, %r, %r)' % (key, r), r['env'])
    else:
        run_row(ctx, key, r)


# widths that end the last strip 2, 4, 16 and 252 columns in (strips of 128 and 256 columns), odd widths (strips of 64)
WIDTHS = [('K3', 'f64', 2, 0, True, True, False, True, 0, False, 128 + 2), ('K3', 'f64', 2, 0, True, True, False, True, 0, False, 256 + 4),
          ('K3', 'f32', 2, 0, True, True, True, True, 0, False, 128 + 16), ('K3', 'f64', 2, 0, True, False, False, False, 0, False, 384 + 2),
          ('K3', 'f32', 4, 0, True, True, False, True, 0, True, 1024 + 4), ('K3', 'f32', 4, 0, True, True, True, True, 0, True, 1024 + 16),
          ('K3', 'f32', 4, 0, True, True, False, True, 0, True, 1024 + 252), ('K3', 'f32', 4, 1, False, True, False, False, 0, False, 1280 + 252),
          ('K3', 'f64', 1, 0, True, True, True, False, 0, False, 64 + 3), ('K3', 'f32', 1, 0, True, False, False, False, 0, False, 64 + 17),
          ('K3', 'f64', 1, 2, False, True, False, False, 0, False, 256 + 61), ('K3-det', 'f64', 1, 0, True, True, False, False, 3, False, 195)]


@pytest.mark.gpu
@pytest.mark.parametrize('w', WIDTHS, ids=['%s-%s-v%d-nx%d' % (w[0], w[1], w[2], w[-1]) for w in WIDTHS])
def test_ragged_last_strip(ctx, w):
    key, nx = w[:-1], w[-1]
    r = dict(row_for(key), nx=nx)
    run_row(ctx, key, r)


@pytest.mark.gpu
@pytest.mark.parametrize('inc,lt,re_', [(True, True, 'xhistogram'), (False, True, 'xhistogram'), (True, False, 'xhistogram'),
                                        (False, False, 'xhistogram'), (True, True, 'numpy'), (False, False, 'numpy')])
def test_directions_and_last_bin_rules(ctx, inc, lt, re_):
    """both `increase`, both `lt`, both last-bin rules, on the chained float64 Keff layout, the E32 layout and the single-read kernel
    (the numpy rule takes FAST off: the chained rows then reach the non-FAST instantiation)"""
    for key in (('K3', 'f64', 2, 0, True, True, True, True, 0, False), ('K3', 'f32', 4, 0, True, True, False, True, 0, True),
                ('K3S', 'f64', True, True, True)):
        r = dict(row_for(key), increase=inc, lt=lt, right_edge=re_)
        if re_ == 'numpy':
            key = key[:7] + (False,) + key[8:] if key[0] == 'K3' else key[:3] + (False,) + key[4:]
            if key[2] == 4:
                key = key[:2] + (2,) + key[3:9] + (False,)            # (the four-cell and E32 variants are FAST only)
        run_row(ctx, key, r)
    for lc in (True, False):
        run_hist(ctx, dict(path='hist', dt='f64', ny=18, nx=130, nslab=2, nint=2, grad=True, det=False, nb=19, last_closed=lc,
                           lt=lt, da='plane', prod_f32=not lt))


def hv(ctx, S, ny, nx, nb, nint=0, det=False):
    """the variant record of one hist call on a stack too large for the exact reference (geometry only)"""
    lat, lon = grid(ny, nx)
    q = tracer(S, ny, nx, np.float64, 0, nan=False)
    rdx, rdy = O.grad_metrics(lat, lon)
    ctx.hist(q, np.linspace(-1.1, 1.1, nb + 1), xvar_dA(ny, nx), [q] * nint, grad=(rdx, rdy, True), deterministic=det, want=('pdf',))
    return ctx.last_hist_variant()


@pytest.mark.gpu
def test_geometry_branches(ctx):
    """the launch geometry each branch of hist_geometry / launch_three is meant to reach"""
    base = dict(path='hist', dt='f64', nint=0, grad=True, det=False, last_closed=True, da='plane')
    v = run_hist(ctx, dict(base, ny=18, nx=130, nslab=2, nb=19))
    assert v['threads'] == 512                                          # half the threads for a small stack
    assert hv(ctx, 64, 128, 512, 19)['threads'] == 1024
    big = run_hist(ctx, dict(base, ny=128, nx=512, nslab=32, nb=19, check_slabs=[0, 31]))
    assert big['bps'] % 8 == 0 and big['xcd_map'] == 1 and big['nchunk'] > 0
    many = run_hist(ctx, dict(base, nint=1, ny=20, nx=130, nslab=2, nb=3000))
    assert many['ncopy'] < 16                                           # many bins x three channels: fewer LDS copies
    tiny = run_hist(ctx, dict(base, ny=2, nx=2, nslab=3, nb=5))
    assert tiny['bps'] == 1 and tiny['nstrip'] == 1                     # the bps clamp: at least one (strip, row) pair per wave
    # det_cap: the deterministic pass caps the rows per wave (many bins: few copies), so it takes more blocks than the default pass
    d = hv(ctx, 16, 2000, 256, 900, nint=1, det=True)
    n = hv(ctx, 16, 2000, 256, 900, nint=1)
    waves = d['threads'] // 64
    cap = 28000 // (waves * (64 // d['ncopy']) * d['vec'])
    assert d['kernel'] == 'K3-det' and cap < 192 and -(-d['nstrip'] * 2000 // (d['bps'] * waves)) <= cap + cap // 16
    assert d['bps'] > n['bps']
    # a base pointer that is not 16-byte aligned: two cells per lane fall to one on an even width
    from xcontour_amd.pipeline import KeffPlan
    rr = dict(path='plan', dt='f64', ny=20, nx=130, N=23, nslab=2, da='land')
    lat, lon = grid(20, 130)
    q = tracer(2, 20, 130, np.float64, 1)
    dA = xvar_dA(20, 130, 'land')
    p = make_plan(ctx, rr, q, dA, lat, lon)
    buf = ctx.alloc(dA.nbytes + 64)
    buf.upload_async(dA, offset_bytes=8)
    ctx.stream_wait_copies()
    p.set_dA_device(buf.ptr + 8)
    p.run()
    v = ctx.last_hist_variant()
    got = p.fetch()
    assert v['vec'] == 1 and v['fast'] == 0 and v['nstrip'] == 3        # (the FAST layout exists with two cells per lane only)
    p.set_dA_device(p.dA_buf.ptr)
    p.run()
    assert ctx.last_hist_variant()['vec'] == 2
    ref = p.fetch()
    for k in ('ctr', 'counts'):
        assert np.array_equal(got[k], ref[k])
    for k in ('area', 'intgrdS'):
        assert np.allclose(got[k], ref[k], rtol=1e-13, atol=0)
    p.free()


@pytest.mark.gpu
@pytest.mark.parametrize('knob,field', [('XC_HIST_XCDMAP', 'xcd_map'), ('XC_HIST_TILEMAP', 'nchunk')])
def test_block_order_knobs(knob, field):
    """XC_HIST_XCDMAP=0 / XC_HIST_TILEMAP=0 (read once, in xc_create: a child process) switch the block / wave order off; the sums
    stay within the exact reference's bound"""
    code = ('r = dict(path="hist", dt="f64", nint=0, grad=True, det=False, last_closed=True, da="plane", ny=128, nx=512, nslab=32, nb=19,'
            ' check_slabs=[0, 31])\nv = T.run_hist(ctx, r)\nassert v[%r] == 0, v\n' % field)
    child(code, {knob: '0'})


@pytest.mark.gpu
def test_a_failed_call_clears_the_record(ctx):
    run_hist(ctx, dict(path='hist', dt='f64', ny=18, nx=130, nslab=2, nint=0, grad=True, det=False, nb=19, last_closed=True, da='plane'))
    assert ctx.last_hist_variant()['kernel'] == 'K3'
    with pytest.raises(Exception):
        ctx.hist(np.zeros((1, 4, 4)), np.array([1.0, 0.0]))             # non monotonic bins
    v = ctx.last_hist_variant()
    assert v['kernel'] is None and all(v[k] == 0 for k in v if k not in ('kernel', 'q_dtype'))


# ------------------------------------------------------------------------------------------------------------------- completeness
def code_object_kernels(tmp):
    """the k_hist / k_keff_single symbols of the gfx950 code objects bundled in the built library"""
    from xcontour_amd import _native as nat
    tool = '/opt/rocm/llvm/bin'
    lib = os.path.join(tmp, 'lib.so')
    shutil.copy(nat.LIB_PATH, lib)
    subprocess.run([os.path.join(tool, 'llvm-objdump'), '--offloading', lib], check=True, cwd=tmp, stdout=subprocess.DEVNULL)
    syms = set()
    for f in sorted(os.listdir(tmp)):
        if 'gfx950' not in f:
            continue
        out = subprocess.run([os.path.join(tool, 'llvm-readelf'), '-Ws', os.path.join(tmp, f)], check=True, stdout=subprocess.PIPE,
                             universal_newlines=True).stdout
        syms |= set(m for m in re.findall(r'\b(_Z\S*(?:k_hist|k_keff_single)\S*)', out) if '.' not in m)     # (not the .kd / .has_* companions)
    return syms


def parse_symbol(s):
    t = {'d': 'f64', 'f': 'f32'}
    m = re.search(r'6k_histI([df])Li(\d)ELi(\d)ELb([01])ELb([01])ELb([01])ELb([01])ELi(\d)ELb([01])EE', s)
    if m:
        g = m.groups()
        det = int(g[7])
        return ('K3' if det == 0 else 'K3-det', t[g[0]], int(g[1]), int(g[2]), g[3] == '1', g[4] == '1', g[5] == '1', g[6] == '1',
                det, g[8] == '1')
    m = re.search(r'13k_keff_singleI([df])Lb([01])ELb([01])ELb([01])EE', s)
    if m:
        g = m.groups()
        return ('K3S', t[g[0]], g[1] == '1', g[2] == '1', g[3] == '1')
    raise AssertionError('unrecognised histogram kernel symbol %s' % s)


UNREACHABLE = {}     # instantiation key -> the reason no public path reaches it (none today)


@pytest.mark.gpu
def test_every_instantiation_has_a_row(tmp_path):
    """every k_hist / k_keff_single instantiation in the gfx950 code object has a row in VARIANTS (or a written reason why it cannot be
    reached), and every row names an instantiation that exists.  Runs no kernel."""
    syms = code_object_kernels(str(tmp_path))
    keys = set(parse_symbol(s) for s in syms)
    assert len(keys) == len(syms) and len(keys) > 100
    rows = set(k for k, _ in ROWS)
    missing = sorted(keys - rows - set(UNREACHABLE), key=str)
    assert not missing, 'instantiations with no row and no reason: %s' % missing
    assert rows <= keys, 'rows for instantiations that do not exist: %s' % sorted(rows - keys, key=str)
    assert len(keys) == len(ALL_KEYS)
