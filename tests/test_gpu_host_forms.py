"""The host forms of the C ABI (xc_forms.hip, xc_keff.hip) called directly through ctypes, pinned on what their staging must not change:
a null optional argument changes no other output (A), a result is the same on each of its three ways home (B), a grown arena changes
nothing (C), nor does XC_COPY_KERNEL=0 (D), and every refusal keeps its code and its text (E).  Inputs on which every sum is exact
(distinct half-integers, weights that are powers of two), so that the comparison is equality of bytes."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from xcontour_amd import _native as nat                                        # noqa: E402

pytestmark = pytest.mark.gpu
P = nat._ptr
S, NY, NX, NC = 2, 5, 7, 3
NONE, ROW, PLANE, SLAB = nat.XC_DA_NONE, nat.XC_DA_ROW, nat.XC_DA_PLANE, nat.XC_DA_SLAB
F32, F64 = nat.XC_F32, nat.XC_F64
E, EE = nat.XC_EBADARG, nat.XC_EEDGES


def code(dt):
    return nat.dtype_code(np.dtype(dt))


def same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), '%s:\n%r\n!=\n%r' % (what, a, b)


class In(object):
    """the inputs of every form on a stack of `s` planes of ny x nx"""

    def __init__(self, dt, s=S, ny=NY, nx=NX, seed=3):
        rng = np.random.default_rng(seed)
        n = s * ny * nx
        self.dt, self.s, self.ny, self.nx = dt, s, ny, nx
        self.q = ((rng.permutation(n) - n // 2) * 0.5).reshape(s, ny, nx).astype(dt) if n <= 4096 \
            else (rng.integers(-35, 36, size=(s, ny, nx)) * 0.5).astype(dt)
        self.f = rng.integers(-8, 9, size=(s, ny, nx)).astype(dt)
        self.y, self.x = np.arange(ny) * 1.0, np.arange(nx) * 1.0
        self.lev = np.array([-10.25, 0.25, 5.25])
        self.w = 2.0 ** rng.integers(-2, 3, size=(ny, nx))
        self.area = np.full((ny, nx), 4.0)
        self.mask = rng.integers(0, 2, size=(ny, nx)).astype(dt)
        self.rdx, self.rdy = 2.0 ** rng.integers(-2, 2, size=ny), 2.0 ** rng.integers(-2, 2, size=ny)
        self.edges = np.arange(-20.0, 20.25, 0.25)


# --------------------------------------------------------------------------------------------------------------- one call per form
# each: (ctx, In, drop=()) -> (return code, {name: output array or None}); `drop` names the optional arguments passed as NULL
def o(drop, name, arr):
    return None if name in drop else arr


def rowsum(c, i, drop=()):
    out = np.empty(i.ny)
    m, w = o(drop, 'mask', i.mask), o(drop, 'dA', i.w)
    rc = c.lib.xc_rowsum(c.handle, P(m), code(i.dt), P(w), PLANE if w is not None else NONE, i.ny, i.nx, 0, P(out))
    return rc, {'rows': out}


def grad2(c, i, drop=()):
    out = np.empty(i.q.shape)
    return c.lib.xc_grad2(c.handle, P(i.q), code(i.dt), i.s, i.ny, i.nx, P(i.rdx), P(i.rdy), 1, P(out)), {'g2': out}


def crossing(c, i, drop=()):
    ln, cn = o(drop, 'out_len', np.empty((i.s, NC))), o(drop, 'out_cnt', np.empty((i.s, NC), dtype=np.uint64))
    rc = c.lib.xc_crossing(c.handle, P(i.q), code(i.dt), i.s, i.ny, i.nx, 0, nat.XC_PAD_EDGE, P(i.lev), NC, 0, P(i.area), F64, 0, 1, 1,
                           P(ln), P(cn))
    return rc, {'out_len': ln, 'out_cnt': cn}


def clen(c, i, drop=(), periodic=False):
    ln, ns = np.empty((i.s, NC)), o(drop, 'out_nseg', np.empty((i.s, NC), dtype=np.uint64))
    head = (c.handle, P(i.q), code(i.dt), i.s, i.ny, i.nx, P(i.y), P(i.x))
    tail = (0.0, P(i.lev), NC, 0, P(ln), P(ns))
    rc = c.lib.xc_contour_lengths_periodic(*head, float(i.nx), *tail) if periodic else c.lib.xc_contour_lengths(*head, *tail)
    return rc, {'out_len': ln, 'out_nseg': ns}


def clen_periodic(c, i, drop=()):
    return clen(c, i, drop, True)


def cline(c, i, drop=()):
    it, ln, ns = np.empty((i.s, NC)), np.empty((i.s, NC)), o(drop, 'out_nseg', np.empty((i.s, NC), dtype=np.uint64))
    rc = c.lib.xc_contour_line_integrals(c.handle, P(i.q), code(i.dt), P(i.f), code(i.dt), i.s, i.ny, i.nx, P(i.y), P(i.x), 0.0, 0.0,
                                         P(i.lev), NC, 0, P(it), P(ln), P(ns))
    return rc, {'out_integral': it, 'out_length': ln, 'out_nseg': ns}


def lclen(c, i, drop=(), periodic=False):
    nwin = ((i.ny + 1) // 2) * ((i.nx + 1) // 2)
    lv = o(drop, 'levels', np.full((i.s, nwin), 0.25))
    ln, le = np.empty((i.s, nwin)), o(drop, 'out_level', np.empty((i.s, nwin)))
    ns = o(drop, 'out_nseg', np.empty((i.s, nwin), dtype=np.uint64))
    head = (c.handle, P(i.q), code(i.dt), i.s, i.ny, i.nx, P(i.y), P(i.x))
    tail = (0.0, 3, 3, 2, 2, 1, P(lv), P(ln), P(le), P(ns))
    rc = c.lib.xc_local_contour_lengths_periodic(*head, float(i.nx), *tail) if periodic else c.lib.xc_local_contour_lengths(*head, *tail)
    return rc, {'out_len': ln, 'out_level': le, 'out_nseg': ns}


def lclen_periodic(c, i, drop=()):
    return lclen(c, i, drop, True)


def cseg(c, i, drop=(), periodic=False):
    """the count-only call (capacity 0: returns 1), then the sized one; the records in a canonical order"""
    fn = c.lib.xc_contour_segments_periodic if periodic else c.lib.xc_contour_segments
    cnt = np.zeros((i.s, NC), dtype=np.uint64)
    args = (c.handle, P(i.q), code(i.dt), i.s, i.ny, i.nx, P(i.lev), NC, 0)
    rc = fn(*args, 0, P(cnt), None, None, None)
    assert rc == 1 and cnt.sum() > 0, 'the count-only call: %d' % rc
    n = int(cnt.sum())
    cnt2, ef, et, pts = np.zeros_like(cnt), np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64), np.empty((n, 4))
    rc = fn(*args, n, P(cnt2), P(ef), P(et), P(pts))
    same(cnt2, cnt, 'counts of the sized call')
    rows = np.column_stack([ef.astype(np.float64), et.astype(np.float64), pts])
    return rc, {'count': cnt, 'records': rows[np.lexsort(rows.T[::-1])]}


def cseg_periodic(c, i, drop=()):
    return cseg(c, i, drop, True)


def minmax(c, i, drop=()):
    out = np.empty((i.s, 2))
    return c.lib.xc_minmax(c.handle, P(i.q), code(i.dt), i.s, i.ny * i.nx, P(out)), {'minmax': out}


def levels(c, i, drop=()):
    mm = np.array([[-17.5, 17.0]] * i.s)
    ctr, ed, st = np.empty((i.s, 9)), np.empty((i.s, 10)), np.empty(i.s, dtype=np.int32)
    rc = c.lib.xc_levels(c.handle, P(mm), code(i.dt), i.s, 9, 1, code(i.dt), nat.XC_EDGE_XHISTOGRAM, P(ctr), P(ed), P(st))
    return rc, {'ctr': ctr, 'edges': ed, 'status': st}


def contours(c, i, drop=()):
    mm, ctr = o(drop, 'out_minmax', np.empty((i.s, 2))), np.empty((i.s, 9))
    ed, st = o(drop, 'out_edges', np.empty((i.s, 10))), o(drop, 'out_status', np.empty(i.s, dtype=np.int32))
    rc = c.lib.xc_contours(c.handle, P(i.q), code(i.dt), i.s, i.ny * i.nx, 9, 1, code(i.dt), nat.XC_EDGE_XHISTOGRAM, P(mm), P(ctr), P(ed), P(st))
    return rc, {'out_minmax': mm, 'ctr': ctr, 'out_edges': ed, 'out_status': st}


def hist(c, i, drop=(), nint=2, grad=1, rank=PLANE):
    d = nat.HistDesc()
    nb = len(i.edges) - 1
    nch = 1 + nint + grad
    w = {NONE: None, ROW: np.ascontiguousarray(i.w[:, 0]), PLANE: i.w, SLAB: np.ascontiguousarray(np.broadcast_to(i.w, i.q.shape))}[rank]
    if rank == ROW:
        w = w.copy()
    d.q, d.q_dtype, d.nslab, d.ny, d.nx = P(i.q), code(i.dt), i.s, i.ny, i.nx
    d.edges, d.nedge, d.last_closed, d.dA, d.dA_rank, d.nint, d.grad, d.lt = P(i.edges), len(i.edges), 1, P(w), rank, nint, grad, 1
    integ = [i.f, np.ascontiguousarray(i.f * 2)]
    for k in range(nint):
        d.integrand[k], d.integrand_dtype[k] = P(integ[k]), code(i.dt)
    if grad:
        d.rdx, d.rdy, d.periodic_x = P(i.rdx), P(i.rdy), 1
    pdf, cdf = o(drop, 'pdf', np.empty((i.s, nch, nb))), o(drop, 'cdf', np.empty((i.s, nch, nb)))
    cnt = o(drop, 'counts', np.empty((i.s, nb), dtype=np.uint64))
    d.pdf, d.cdf, d.counts = P(pdf), P(cdf), P(cnt)
    return c.lib.xc_hist(c.handle, C.byref(d)), {'pdf': pdf, 'cdf': cdf, 'counts': cnt}


VECTORS = ('area', 'intgrdS', 'latEq', 'dqdA', 'dintSdA', 'Leq2', 'Lmin', 'nkeff')


def epilogue(c, i, drop=(), npre=3):
    N, ntbl = 9, 6
    rng = np.random.default_rng(11)
    pdf = rng.integers(1, 9, size=(i.s, 2, N)).astype(np.float64)
    ctr = np.ascontiguousarray(np.broadcast_to(np.arange(N) * 0.5, (i.s, N)))
    tbl, crd = np.arange(ntbl) * 16.0, np.linspace(-80.0, 80.0, ntbl)
    pre = o(drop, 'preY', np.array([-40.0, 0.0, 40.0])) if npre else None
    out = {k: o(drop, k, np.empty((i.s, N))) for k in VECTORS}
    out['interp'] = o(drop, 'interp', np.empty((i.s, 9, npre))) if npre else None
    rc = c.lib.xc_keff_epilogue(c.handle, P(pdf), P(ctr), F64, i.s, N, 1, 1, P(tbl), P(crd), ntbl, P(pre), npre, 1e5, 2.0 * np.pi * 6371200.0,
                                *[P(out[k]) for k in VECTORS], P(out['interp']))
    return rc, out


def lwa(c, i, drop=(), nmask=2):
    Q = np.ascontiguousarray(np.broadcast_to(np.linspace(-12.0, 12.0, i.ny), (i.s, i.ny)))
    M = o(drop, 'M', np.ones((i.ny, i.nx)))
    mi = np.array([1, 3], dtype=np.int32) if nmask else None
    out, mo = np.empty(i.q.shape), (np.empty((i.s, nmask, i.ny, i.nx), dtype=np.int8) if nmask else None)
    assert c.lib.xc_set_lwa_exact(c.handle, 1) == 0                              # the band walk: numpy's own order of summation
    rc = c.lib.xc_lwa(c.handle, P(i.q), code(i.dt), P(Q), P(i.y), P(i.w), PLANE, 4.0, P(M), PLANE if M is not None else NONE, i.s, i.ny, i.nx,
                      1, 0, 0, P(mi), nmask, P(out), P(mo))
    c.lib.xc_set_lwa_exact(c.handle, 0)
    return rc, {'lwa': out, 'masks': mo}


def sort(c, i, drop=()):
    n, J, ntbl = i.ny * i.nx, 0 if 'out_Q' in drop else 4, 6
    mask = o(drop, 'mask', np.ones((i.ny, i.nx), dtype=i.dt))
    tg = np.array([4.0, 16.0, 32.0, 48.0]) if J else None
    tbl, crd = np.arange(ntbl) * 16.0, np.linspace(-80.0, 80.0, ntbl)
    Q, qs, ac = o(drop, 'out_Q', np.empty((i.s, 4))), o(drop, 'out_qsorted', np.empty((i.s, n))), o(drop, 'out_acum', np.empty((i.s, n)))
    nv, bpe = o(drop, 'out_nvalid', np.zeros(i.s, dtype=np.uint32)), o(drop, 'out_bpe', np.zeros(i.s))
    if bpe is None:
        tbl = crd = None
    rc = c.lib.xc_sort_profile_batch(c.handle, P(i.q), code(i.dt), P(mask), code(i.dt), 0, P(i.w), PLANE, i.s, i.ny, i.nx, 0, P(tg), J,
                                     P(tbl), P(crd), ntbl if tbl is not None else 0, P(Q), P(qs), P(ac), P(nv), P(bpe))
    return rc, {'out_Q': Q, 'out_qsorted': qs, 'out_acum': ac, 'out_nvalid': nv, 'out_bpe': bpe}


# form -> the optional arguments that may be NULL one at a time without changing any other output (a neutral input: a mask of ones)
FORMS = [(rowsum, ()), (grad2, ()), (crossing, ('out_len', 'out_cnt')), (clen, ('out_nseg',)), (clen_periodic, ('out_nseg',)),
         (cline, ('out_nseg',)), (lclen, ('out_level', 'out_nseg')), (lclen_periodic, ('out_level', 'out_nseg')), (cseg, ()),
         (cseg_periodic, ()), (minmax, ()), (levels, ()), (contours, ('out_minmax', 'out_edges', 'out_status')),
         (hist, ('pdf', 'cdf', 'counts')), (epilogue, VECTORS + ('interp',)), (lwa, ()),
         (sort, ('mask', 'out_Q', 'out_qsorted', 'out_acum', 'out_nvalid', 'out_bpe'))]


def ok(call, *a, **k):
    rc, out = call(*a, **k)
    assert rc == 0, '%s: %d %r' % (call.__name__, rc, a[0].lib.xc_last_error(a[0].handle))
    return out


def compare(full, got, what, skip=()):
    for k, v in got.items():
        if v is not None and k not in skip:
            same(v, full[k], '%s: %s' % (what, k))


def pdf0_ref(i):
    """channel 0 of xc_hist: the weights summed per bin, np.digitize's bins with the last edge closed, cells outside dropped"""
    nb = len(i.edges) - 1
    x = i.q.astype(np.float64).reshape(i.s, -1)
    idx = np.where(x == i.edges[-1], nb - 1, np.digitize(x, i.edges) - 1)
    w = i.w.ravel()
    return np.stack([np.bincount(idx[s][(idx[s] >= 0) & (idx[s] < nb)], weights=w[(idx[s] >= 0) & (idx[s] < nb)], minlength=nb) for s in range(i.s)])


# ------------------------------------------------------------------------------------------------------------------------- case A
@pytest.mark.parametrize('dt', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('form', FORMS, ids=[f[0].__name__ for f in FORMS])
def test_a_null_argument_changes_no_other_output(ctx, form, dt):
    call, optional = form
    i = In(dt)
    full = ok(call, ctx, i)
    assert all(v is not None for v in full.values())
    for name in optional:
        compare(full, ok(call, ctx, i, drop=(name,)), '%s without %s' % (call.__name__, name))
    compare(full, ok(call, ctx, i), call.__name__ + ' again')


@pytest.mark.parametrize('dt', [np.float32, np.float64], ids=['f32', 'f64'])
def test_a_variants_that_change_the_sums(ctx, dt):
    """the optional inputs and counts that change what is computed, each against numpy or against the outputs they leave alone"""
    i = In(dt)
    # xc_rowsum: where(mask == 1) of the weights, all of them without a mask, ones without weights
    want = lambda m, w: np.where(m == 1, w, 0.0).sum(axis=1)
    one = np.ones((NY, NX))
    same(ok(rowsum, ctx, i)['rows'], want(i.mask, i.w), 'rowsum')
    same(ok(rowsum, ctx, i, drop=('mask',))['rows'], want(one, i.w), 'rowsum without a mask')
    same(ok(rowsum, ctx, i, drop=('dA',))['rows'], want(i.mask, one), 'rowsum without weights')
    # xc_local_contour_lengths without levels: consistent whichever outputs are asked for
    for call in (lclen, lclen_periodic):
        base = ok(call, ctx, i, drop=('levels',))
        for name in ('out_level', 'out_nseg'):
            compare(base, ok(call, ctx, i, drop=('levels', name)), '%s without levels and %s' % (call.__name__, name))
    # xc_hist: channel 0 (the weights) whatever other channels ride along and whatever rank states the same weights
    full = ok(hist, ctx, i)
    same(np.ascontiguousarray(full['pdf'][:, 0]), pdf0_ref(i), 'hist channel 0')
    for nint in (0, 1, 2):
        for grad in (0, 1):
            got = ok(hist, ctx, i, nint=nint, grad=grad)
            assert got['pdf'].shape[1] == 1 + nint + grad
            for k in ('pdf', 'cdf'):
                same(np.ascontiguousarray(got[k][:, :1 + nint]), np.ascontiguousarray(full[k][:, :1 + nint]), 'hist nint %d grad %d %s' % (nint, grad, k))
            same(got['counts'], full['counts'], 'hist counts')
    i.w[:] = i.w[:, :1]                                                         # (weights a row can state)
    plane = ok(hist, ctx, i)
    for rank in (ROW, SLAB):
        compare(plane, ok(hist, ctx, i, rank=rank), 'hist dA_rank %d' % rank)
    none = ok(hist, ctx, i, rank=NONE, nint=0, grad=0)
    same(np.ascontiguousarray(none['pdf'][:, 0]), none['counts'].astype(np.float64), 'hist without weights counts cells')
    # xc_keff_epilogue: the eight vectors with and without the interpolation
    full = ok(epilogue, ctx, i)
    compare(full, ok(epilogue, ctx, i, npre=0), 'epilogue npre 0')
    compare(full, ok(epilogue, ctx, i, drop=('interp',)), 'epilogue npre 3 without interp')
    # xc_lwa: the activity with and without the masks, under a metric M and without one
    for drop in ((), ('M',)):
        compare(ok(lwa, ctx, i, drop=drop), ok(lwa, ctx, i, drop=drop, nmask=0), 'lwa nmask 0 %r' % (drop,))


# ------------------------------------------------------------------------------------------------------------------------- case B
def grad2_ref(q, rdx, rdy):
    q = q.astype(np.float64)
    gx = (np.roll(q, -1, axis=2) - np.roll(q, 1, axis=2)) * rdx[None, :, None]
    ny = q.shape[1]
    jn, js = np.minimum(np.arange(ny) + 1, ny - 1), np.maximum(np.arange(ny) - 1, 0)
    gy = (q[:, jn, :] - q[:, js, :]) * rdy[None, :, None]
    return gx * gx + gy * gy


def test_b_every_transport_path_of_a_result(ctx):
    """below XC_COPY_OUT_KB (written straight into the pinned buffer), up to 1 MiB (pinned bounce), above (plain copy)"""
    kb = int(os.environ.get('XC_COPY_OUT_KB', 256))
    for n in (8, 200, 400):
        i = In(np.float64, 1, n, n)
        got = ok(grad2, ctx, i)['g2']
        assert (got.nbytes <= kb << 10, got.nbytes <= 1 << 20) == {8: (True, True), 200: (False, True), 400: (False, False)}[n]
        same(got, grad2_ref(i.q, i.rdx, i.rdy), 'grad2 %d x %d' % (n, n))
    for s in (4, 256, 1024):
        i = In(np.float32, s)
        got = ok(hist, ctx, i, drop=('cdf', 'counts'), nint=0, grad=0)['pdf']
        assert (got.nbytes <= kb << 10, got.nbytes <= 1 << 20) == {4: (True, True), 256: (False, True), 1024: (False, False)}[s]
        same(got, pdf0_ref(i)[:, None, :], 'hist pdf of %d slabs' % s)


# ------------------------------------------------------------------------------------------------------------------------- case C
def test_c_arena_growth_changes_nothing():
    c = nat.Context(0)
    try:
        small, big = In(np.float32), In(np.float64, 1, 400, 400)
        before = [ok(grad2, c, small), ok(clen, c, small)]
        g, l = ok(grad2, c, big), ok(clen, c, big)
        same(g['g2'], grad2_ref(big.q, big.rdx, big.rdy), 'the large grad2')
        assert l['out_nseg'].sum() > 0
        after = [ok(grad2, c, small), ok(clen, c, small)]
        for b, a in zip(before, after):
            compare(b, a, 'after the arena grew')
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------------------------------- case D
def digest(c):
    h = hashlib.sha256()
    i = In(np.float64)
    for call, _ in FORMS:
        for k, v in sorted(ok(call, c, i).items()):
            h.update(k.encode()); h.update(v.tobytes())
    return h.hexdigest()


def test_d_copy_kernel_off(ctx):
    env = dict(os.environ, XC_COPY_KERNEL='0')
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert r.stdout.strip().splitlines()[-1] == 'digest ' + digest(ctx), r.stdout


# ------------------------------------------------------------------------------------------------------------------------- case E
def refused(c, rc, want_rc, text):
    assert rc == want_rc and c.lib.xc_last_error(c.handle) == text.encode(), (rc, c.lib.xc_last_error(c.handle), text)


def test_e_refusals(ctx):
    c, L, h = ctx, ctx.lib, ctx.handle
    i = In(np.float64)
    q, y, x, lev, out = P(i.q), P(i.y), P(i.x), P(i.lev), P(np.empty(4096))
    bad_y, desc = np.array([0.0, 1.0, np.inf, 3.0, 4.0]), np.array([1.0, 0.0, 2.0])        # (named: the arrays must outlive the calls)
    bad_x, zeros, past, bad_edges = np.array([0.0, 1.0, 2.0, np.nan, 4.0, 5.0, 6.0]), np.zeros((S, NY)), np.array([NY], dtype=np.int32), np.array([0.0, 2.0, 1.0])
    shape = (S, NY, NX)
    # K2, K4
    refused(c, L.xc_rowsum(h, P(i.mask), F64, P(i.w), PLANE, NY, NX, 0, None), E, 'xc_rowsum: bad arguments')
    refused(c, L.xc_rowsum(h, P(i.mask), 2, P(i.w), PLANE, NY, NX, 0, out), E, 'xc_rowsum: bad mask dtype')
    refused(c, L.xc_rowsum(h, P(i.mask), F64, None, ROW, NY, NX, 0, out), E, 'xc_rowsum: dA is NULL')
    refused(c, L.xc_grad2(h, q, F64, 0, NY, NX, P(i.rdx), P(i.rdy), 1, out), E, 'xc_grad2: bad arguments')
    refused(c, L.xc_grad2(h, q, 2, *shape, P(i.rdx), P(i.rdy), 1, out), E, 'xc_grad2: bad dtype')
    # K9
    cr = lambda qd=F64, ad=F64, cs=lev, ol=out: L.xc_crossing(h, q, qd, *shape, 0, 0, cs, NC, 0, P(i.area), ad, 0, 1, 1, ol, None)
    refused(c, cr(ol=None), E, 'xc_crossing: bad arguments')
    refused(c, cr(ad=2), E, 'xc_crossing: bad dtype')
    refused(c, cr(cs=P(desc)), EE, 'xc_crossing: contours must be ascending without NaN')
    # K10
    cl = lambda qd=F64, yy=y, r=0.0, cs=lev: L.xc_contour_lengths(h, q, qd, *shape, yy, x, r, cs, NC, 0, out, None)
    refused(c, cl(cs=None), E, 'xc_contour_lengths: bad arguments')
    refused(c, cl(qd=2), E, 'xc_contour_lengths: bad dtype')
    refused(c, cl(r=-1.0), E, 'xc_contour_lengths: radius must be >= 0')
    refused(c, cl(yy=P(bad_y)), E, 'xc_contour_lengths: coordinates must be finite')
    refused(c, cl(cs=P(desc)), EE, 'xc_contour_lengths: contours must be ascending without NaN')
    refused(c, L.xc_contour_lengths_periodic(h, q, F64, *shape, y, x, 6.0, 0.0, lev, NC, 0, out, None), E,
            'xc_contour_lengths_periodic: period must be finite, non-zero, of the sign of xcoord[nx-1] - xcoord[0] and longer than that span, '
            'and nx >= 2')
    # K15
    ci = lambda qd=F64, fd=F64, xx=x, r=0.0, per=0.0, cs=lev: L.xc_contour_line_integrals(h, q, qd, P(i.f), fd, *shape, y, xx, per, r, cs, NC, 0,
                                                                                        out, out, None)
    refused(c, ci(cs=None), E, 'xc_contour_line_integrals: bad arguments')
    refused(c, ci(fd=2), E, 'xc_contour_line_integrals: bad dtype')
    refused(c, ci(r=-1.0), E, 'xc_contour_line_integrals: radius must be >= 0')
    refused(c, ci(xx=P(bad_x)), E, 'xc_contour_line_integrals: coordinates must be finite')
    refused(c, ci(per=-7.0), E, 'xc_contour_line_integrals: period must be 0, or finite, of the sign of xcoord[nx-1] - xcoord[0] and longer '
                                'than that span, and nx >= 2')
    refused(c, ci(cs=P(desc)), EE, 'xc_contour_line_integrals: contours must be ascending without NaN')
    # K11
    lc = lambda qd=F64, yy=y, wy=3, sy=2: L.xc_local_contour_lengths(h, q, qd, *shape, yy, x, 0.0, wy, 3, sy, 2, 1, None, out, None, None)
    refused(c, L.xc_local_contour_lengths(h, q, F64, *shape, y, x, 0.0, 3, 3, 2, 2, 1, None, None, None, None), E,
            'xc_local_contour_lengths: bad arguments')
    refused(c, lc(qd=2), E, 'xc_local_contour_lengths: bad dtype')
    refused(c, lc(wy=1), E, 'xc_local_contour_lengths: the window must be at least 2 x 2 nodes')
    refused(c, lc(sy=0), E, 'xc_local_contour_lengths: strides must be >= 1')
    refused(c, lc(yy=P(bad_y)), E, 'xc_local_contour_lengths: coordinates must be finite')
    lp = lambda per, wx: L.xc_local_contour_lengths_periodic(h, q, F64, *shape, y, x, per, 0.0, 3, wx, 2, 2, 1, None, out, None, None)
    refused(c, lp(6.0, 3), E, 'xc_local_contour_lengths_periodic: period must be finite, non-zero, of the sign of xcoord[nx-1] - xcoord[0] '
                              'and longer than that span, and nx >= 2')
    refused(c, lp(7.0, 8), E, 'xc_local_contour_lengths_periodic: the window must not be wider than the ring (wx <= nx)')
    # K12
    cs_ = lambda qd=F64, cap=0, cs=lev, fn=L.xc_contour_segments, nx=NX: fn(h, q, qd, S, NY, nx, cs, NC, 0, cap, out, None, None, None)
    refused(c, cs_(cap=-1), E, 'xc_contour_segments: bad arguments')
    refused(c, cs_(fn=L.xc_contour_segments_periodic, nx=1), E, 'xc_contour_segments_periodic: nx >= 2')
    refused(c, cs_(qd=2), E, 'xc_contour_segments: bad dtype')
    refused(c, cs_(cap=5), E, 'xc_contour_segments: capacity > 0 needs the record arrays')
    refused(c, cs_(cs=P(desc)), EE, 'xc_contour_segments: contours must be ascending without NaN')
    # K7
    lw = lambda qd=F64, nm=0, mi=None: L.xc_lwa(h, q, qd, P(zeros), y, P(i.w), PLANE, 4.0, None, NONE, *shape, 1, 0, 0, mi, nm, out, out)
    refused(c, L.xc_lwa(h, q, F64, None, y, P(i.w), PLANE, 4.0, None, NONE, *shape, 1, 0, 0, None, 0, out, None), E, 'xc_lwa: bad arguments')
    refused(c, lw(qd=2), E, 'xc_lwa: bad dtype')
    refused(c, lw(nm=1), E, 'xc_lwa: mask arguments')
    refused(c, lw(nm=1, mi=P(past)), E, 'indices in mask_idx out of boundary')
    # K8
    so = lambda qd=F64, md=F64, da=P(i.w), J=0, bpe=None: L.xc_sort_profile_batch(h, q, qd, P(i.mask), md, 0, da, PLANE, *shape, 0, None, J,
                                                                                 None, None, 0, None, out, None, None, bpe)
    refused(c, so(J=-1), E, 'xc_sort_profile: bad arguments')
    refused(c, so(qd=2), E, 'xc_sort_profile: bad dtype')
    refused(c, so(md=2), E, 'xc_sort_profile: bad mask dtype')
    refused(c, so(da=None), E, 'xc_sort_profile: dA is NULL')
    refused(c, so(bpe=out), E, 'xc_sort_profile: BPE needs tbl/coord')
    assert L.xc_sync(h) == 0                                                     # (that refusal comes after the first copies)
    # K1, the levels
    refused(c, L.xc_minmax(h, q, F64, S, 0, out), E, 'xc_minmax: bad arguments')
    refused(c, L.xc_minmax(h, q, 2, S, NY * NX, out), E, 'xc_minmax: q_dtype must be XC_F32 or XC_F64')
    refused(c, L.xc_levels(h, out, F64, S, 1, 1, F64, 1, out, out, out), E, 'xc_levels: bad arguments (need N >= 2)')
    refused(c, L.xc_contours(h, q, F64, S, NY * NX, 9, 1, F64, 1, None, None, None, None), E, 'xc_contours: bad arguments (need N >= 2)')
    refused(c, L.xc_contours(h, q, 2, S, NY * NX, 9, 1, F64, 1, None, out, None, None), E, 'xc_contours: q_dtype must be XC_F32 or XC_F64')
    # K3
    refused(c, L.xc_hist(h, None), E, 'xc_hist: desc is NULL')
    refused(c, L.xc_hist(h, C.byref(nat.HistDesc())), E, 'xc_hist: q / edges is NULL')

    def hd(edges=bad_edges, integ=(), **kw):
        """a descriptor with nothing wrong but its edges, then the fields named"""
        d = nat.HistDesc()
        d.q, d.q_dtype, d.nslab, d.ny, d.nx, d.edges, d.nedge, d.pdf = q, F64, S, NY, NX, P(edges), len(edges), out
        for k, v in enumerate(integ):
            d.integrand[k], d.integrand_dtype[k] = v
        for k, v in kw.items():
            setattr(d, k, v)
        return L.xc_hist(h, C.byref(d))
    refused(c, hd(), EE, 'non monotonic bins')
    refused(c, hd(q_dtype=2), E, 'xc_hist: q_dtype must be XC_F32 or XC_F64')
    refused(c, hd(ny=0), E, 'xc_hist: nslab, ny, nx must be >= 1')
    refused(c, hd(nedge=1), E, 'xc_hist: need at least 2 edges')
    refused(c, hd(dA_rank=SLAB + 1), E, 'xc_hist: bad dA_rank')
    refused(c, hd(dA_rank=ROW), E, 'xc_hist: dA is NULL')
    refused(c, hd(nint=3), E, 'xc_hist: nint must be 0..2')
    refused(c, hd(nint=1), E, 'xc_hist: integrand is NULL')
    refused(c, hd(nint=1, integ=[(q, 2)]), E, 'xc_hist: bad integrand dtype')
    refused(c, hd(grad=1, rdx=out), E, 'xc_hist: grad needs rdx and rdy')
    refused(c, hd(grad=1, rdx=out, rdy=out, negate=1), E, 'xc_hist: negate is not available together with grad')
    refused(c, hd(pdf=None), E, 'xc_hist: no output requested')
    # K5 / K6: the late refusal comes after the takes
    ep = lambda N=9, npre=0, pre=None, itp=None: L.xc_keff_epilogue(h, out, out, F64, S, N, 1, 1, out, out, 6, pre, npre, 1e5, 1.0,
                                                                  out, None, None, None, None, None, None, None, itp)
    refused(c, ep(N=1), E, 'xc_keff_epilogue: bad arguments')
    refused(c, ep(npre=3, itp=out), E, 'xc_keff_epilogue: preY is NULL')
    assert L.xc_sync(h) == 0
    # ... and the context still works
    compare(ok(grad2, c, i), {'g2': grad2_ref(i.q, i.rdx, i.rdy)}, 'after the refusals')


if __name__ == '__main__':                                                       # case D's child: XC_COPY_KERNEL is read when the context is made
    ctx_ = nat.Context(0)
    print('digest ' + digest(ctx_))
    ctx_.close()
