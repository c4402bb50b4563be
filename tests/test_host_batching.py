# -*- coding: utf-8 -*-
"""How `_native.Context` cuts a stack into batches, pinned without a GPU: a Context over a stand-in library that records
(entry point, nslab) per call.  The batch boundaries, the order of the library calls, the container shape of every joined result
and the reads of a lazy stack (every slab once, in order) are what a change to the batching must leave alone."""
import ctypes as C

import numpy as np
import pytest

from xcontour_amd import _native as nat
from xcontour_amd import labeled as lb

S, NY, NX, N = 5, 6, 8, 4
SLAB = NY * NX * 8                      # bytes of one float64 slab

# position of `nslab` in the argument list of the entry points that take it by value (include/xcontour_hip.h)
_NSLAB_ARG = {'xc_minmax': 3, 'xc_levels': 3, 'xc_contours': 3, 'xc_grad2': 3, 'xc_crossing': 3, 'xc_crossing_dev': 3,
              'xc_contour_lengths': 3, 'xc_contour_lengths_dev': 3, 'xc_lwa': 10, 'xc_sort_profile_batch': 8}


class _Lib(object):
    """every xc_* entry point returns XC_OK and leaves its outputs alone; compute entry points are recorded"""

    def __init__(self):
        self.calls = []
        self._next = 1 << 40

    def __getattr__(self, name):
        if name == 'xc_malloc':
            return self._malloc
        if name == 'xc_memcpy_d2h':
            return lambda h, dst, src, n: (C.memset(dst, 0, n), 0)[1]
        if name == 'xc_hist':
            return lambda h, dref: (self.calls.append((name, int(dref._obj.nslab))), 0)[1]
        if name in _NSLAB_ARG:
            return lambda *a: (self.calls.append((name, int(a[_NSLAB_ARG[name]]))), 0)[1]
        return lambda *a: 0

    def _malloc(self, h, n, pref):
        pref._obj.value = self._next
        self._next += (int(n) + 4095) & ~4095
        return 0


@pytest.fixture
def ctx():
    c = nat.Context.__new__(nat.Context)
    c.lib, c.handle, c.device = _Lib(), None, 0
    c._buffers, c._resident, c._staged, c._ev_pool = [], {}, [], []
    c.max_batch_bytes = 2 * SLAB + 8
    return c


@pytest.fixture
def q():
    return np.random.default_rng(7).standard_normal((S, NY, NX))


def _calls(ctx):
    out, ctx.lib.calls = ctx.lib.calls, []
    return out


def _seq(name, *ns):
    return [(name, n) for n in ns]


def test_minmax_and_contours_batches(ctx, q):
    mm = ctx.minmax(q)
    assert _calls(ctx) == _seq('xc_minmax', 2, 2, 1)
    assert type(mm) is np.ndarray and mm.shape == (S, 2) and mm.dtype == np.float64
    ctr = ctx.contours(q, N, True, np.float32)
    assert _calls(ctx) == _seq('xc_minmax', 2, 2, 1) + _seq('xc_levels', S)
    assert type(ctr) is np.ndarray and ctr.shape == (S, N)
    res = ctx.contours(q, N, True, np.float32, want_minmax=True)
    assert _calls(ctx) == _seq('xc_minmax', 2, 2, 1) + _seq('xc_levels', S)
    assert type(res) is tuple and res[0].shape == (S, N) and res[1].shape == (S, 2)
    ctx.max_batch_bytes = 8 << 30                                   # everything fits: the one-call form
    res = ctx.contours(q, N, True, np.float32, want_minmax=True)
    assert _calls(ctx) == _seq('xc_contours', S)
    assert type(res) is tuple and res[0].shape == (S, N) and res[1].shape == (S, 2)


def test_hist_batches(ctx, q):
    edges = np.linspace(-3, 3, N + 1)
    out = ctx.hist(q, edges)
    assert _calls(ctx) == _seq('xc_hist', 2, 2, 1)
    assert type(out) is dict and list(out) == ['pdf', 'cdf', 'counts']
    assert out['pdf'].shape == out['cdf'].shape == (S, 1, N) and out['counts'].shape == (S, N) and out['counts'].dtype == np.uint64
    # per-slab edges, per-slab weights and one integrand: 3 x 8 bytes per cell staged, one slab per batch
    out = ctx.hist(q, np.tile(edges, (S, 1)), dA=np.ones((S, NY, NX)), integrands=[q * 2.0], want=('cdf',))
    assert _calls(ctx) == _seq('xc_hist', 1, 1, 1, 1, 1)
    assert type(out) is dict and list(out) == ['cdf'] and out['cdf'].shape == (S, 2, N)


def test_grad2_batches(ctx, q):
    g = ctx.grad2(q, np.ones(NY), np.ones(NY))
    assert _calls(ctx) == _seq('xc_grad2', 1, 1, 1, 1, 1)          # tracer + the float64 result: 2 x 8 bytes per cell
    assert type(g) is np.ndarray and g.shape == (S, NY, NX) and g.dtype == np.float64


def test_crossing_batches(ctx, q):
    levels = np.linspace(-1, 1, N)
    res = ctx.crossing(q, levels, np.ones((NY, NX)))
    assert _calls(ctx) == _seq('xc_crossing', 2, 2, 1)
    assert type(res) is tuple and len(res) == 2
    assert res[0].shape == res[1].shape == (S, N) and res[0].dtype == np.float64 and res[1].dtype == np.uint64
    # several strides: both strides of a batch on its one upload, before the next batch
    res = ctx.crossing(q, np.tile(levels, (S, 1)), np.ones((NY, NX)), stride=[1, 2])
    assert _calls(ctx) == _seq('xc_crossing_dev', 2, 2, 2, 2, 1, 1)
    assert type(res) is list and len(res) == 2
    for r in res:
        assert type(r) is tuple and r[0].shape == r[1].shape == (S, N) and r[0].dtype == np.float64 and r[1].dtype == np.uint64
    assert ctx._buffers == []                                       # the temporaries of every batch were freed


def test_contour_lengths_batches(ctx, q):
    res = ctx.contour_lengths(q, np.linspace(-1, 1, N), np.arange(NY, dtype=float), np.arange(NX, dtype=float))
    assert _calls(ctx) == _seq('xc_contour_lengths', 2, 2, 1)
    assert type(res) is tuple and len(res) == 2
    assert res[0].shape == res[1].shape == (S, N) and res[0].dtype == np.float64 and res[1].dtype == np.uint64


def test_lwa_batches(ctx, q):
    Q = np.sort(q[:, :, 0], axis=1)
    out, masks = ctx.lwa(q, Q, np.arange(NY, dtype=float), np.ones(NY), 1.0)
    assert _calls(ctx) == _seq('xc_lwa', 1, 1, 1, 1, 1)            # tracer + the float64 result
    assert out.shape == (S, NY, NX) and out.dtype == np.float64 and masks is None
    out, masks = ctx.lwa(q, Q, np.arange(NY, dtype=float), np.ones((NY, NX)), 1.0, M=np.ones(NY), mask_idx=[1, 3], exact=False)
    assert _calls(ctx) == _seq('xc_lwa', 1, 1, 1, 1, 1)
    assert out.shape == (S, NY, NX) and masks.shape == (S, 2, NY, NX) and masks.dtype == np.int8


def test_sort_profile_batches(ctx, q):
    ctx.max_batch_bytes = 2 * NY * NX * 40 + 8                      # tracer + the sort's four work arrays: 40 bytes per cell
    out = ctx.sort_profile(q, dA=np.ones(NY), targets=np.array([0.5, 1.5, 2.5]), tbl=np.arange(NY, dtype=float),
                           coord=np.arange(NY, dtype=float))
    assert _calls(ctx) == _seq('xc_sort_profile_batch', 2, 2, 1)
    assert type(out) is dict and list(out) == ['nvalid', 'Q', 'bpe']
    assert out['nvalid'].shape == (S,) and out['nvalid'].dtype == np.int64 and out['Q'].shape == (S, 3) and out['bpe'].shape == (S,)
    ctx.max_batch_bytes = 2 * NY * NX * 72 + 8                      # + both full-length outputs, a per-slab mask and per-slab weights
    out = ctx.sort_profile(q, dA=np.ones((S, NY, NX)), mask=np.ones((S, NY, NX)), want_sorted=True, want_acum=True)
    assert _calls(ctx) == _seq('xc_sort_profile_batch', 2, 2, 1)
    assert list(out) == ['nvalid', 'q_sorted', 'acum'] and out['q_sorted'].shape == out['acum'].shape == (S, NY * NX)
    # one plane in, scalars / 1-D arrays out
    out = ctx.sort_profile(q[0], targets=np.array([0.5, 1.5]), tbl=np.arange(NY, dtype=float), coord=np.arange(NY, dtype=float),
                           want_sorted=True)
    assert _calls(ctx) == _seq('xc_sort_profile_batch', 1)
    assert type(out['nvalid']) is int and type(out['bpe']) is float and out['Q'].shape == (2,) and out['q_sorted'].shape == (NY * NX,)


class _Source(object):
    """a lazy (S, ny, nx) source that records which slabs every read asks for"""

    def __init__(self, a):
        self.a, self.shape, self.dtype, self.reads = a, a.shape, a.dtype, []

    def __getitem__(self, key):
        self.reads.append(tuple(range(*key[0].indices(self.shape[0]))))
        return self.a[key]


def _lazy(q):
    src = _Source(q)
    return src, lb.LazyStack(src, [0], 1, 2)


@pytest.mark.parametrize('method', ['minmax', 'contours', 'hist', 'grad2', 'crossing', 'crossing_strides', 'contour_lengths', 'lwa',
                                    'sort_profile'])
def test_a_lazy_stack_is_read_batch_by_batch_every_slab_once_in_order(ctx, q, method):
    src, st = _lazy(q)
    levels = np.linspace(-1, 1, N)
    one_by_one = [(0,), (1,), (2,), (3,), (4,)]
    pairs = [(0, 1), (2, 3), (4,)]
    if method == 'minmax':
        out, want = ctx.minmax(st), pairs
    elif method == 'contours':
        out, want = ctx.contours(st, N, True, np.float64), pairs
    elif method == 'hist':
        src2, st2 = _lazy(q * 2.0)
        out, want = ctx.hist(st, np.linspace(-3, 3, N + 1), integrands=[st2], want=('cdf',))['cdf'], one_by_one
        assert src2.reads == want                                   # the lazy integrand too
    elif method == 'grad2':
        out, want = ctx.grad2(st, np.ones(NY), np.ones(NY)), one_by_one
    elif method == 'crossing':
        out, want = ctx.crossing(st, levels, np.ones((NY, NX)))[0], pairs
    elif method == 'crossing_strides':
        out, want = ctx.crossing(st, levels, np.ones((NY, NX)), stride=[1, 2])[1][0], pairs
    elif method == 'contour_lengths':
        out, want = ctx.contour_lengths(st, levels, np.arange(NY, dtype=float), np.arange(NX, dtype=float))[0], pairs
    elif method == 'lwa':
        out, want = ctx.lwa(st, np.sort(q[:, :, 0], axis=1), np.arange(NY, dtype=float), np.ones(NY), 1.0)[0], one_by_one
    else:
        ctx.max_batch_bytes = 2 * NY * NX * 40 + 8
        out, want = ctx.sort_profile(st, targets=np.array([0.5]))['Q'], pairs
    assert src.reads == want
    assert out.shape[0] == S
    # everything in one batch: one read of the whole stack
    src.reads[:] = []
    ctx.max_batch_bytes = 8 << 30
    ctx.minmax(st)
    assert src.reads == [tuple(range(S))]
