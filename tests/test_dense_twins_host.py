# -*- coding: utf-8 -*-
"""One argument list for both forms of the dense contour calls, pinned without a GPU: every `Context` method with a host entry and a
`_dev` twin (K10, K11, K15, K25, K26 and `coarsen`) is run over the stand-in library twice, without and with a device mirror of the
tracer, on the 5-slab stack that test_host_batching.py cuts into batches of 2, 2 and 1.  What the `_dev` entry is handed must be what
the host entry is handed, pointer for pointer: the tracer at its mirror, every small array and every output at the allocation made for
it, in order."""
import ctypes as C

import numpy as np
import pytest

import standin_lib
from standin_lib import DEV, RES, _Lib

from xcontour_amd import _native as nat

S, NY, NX, N = 5, 6, 8, 4
SLAB = NY * NX * 8                      # bytes of one float64 slab
BATCHES = [(0, 2), (2, 2), (4, 1)]      # (first slab, slabs)
Y, X = np.arange(NY, dtype=float), np.arange(NX, dtype=float)
PERIOD, RADIUS = float(NX), 2.5
WIN, STR, NWIN = (3, 4), (2, 3), 3 * 3  # K11: windows of 3 x 4 nodes every 2 rows / 3 columns: ceil(6 / 2) x ceil(8 / 3) of them
Q = np.random.default_rng(7).standard_normal((S, NY, NX))
F = np.random.default_rng(8).standard_normal((S, NY, NX))
LEVELS = np.linspace(-1, 1, N)[None, :] + 0.01 * np.arange(S)[:, None]          # per slab
VALUES = [np.arange(N, dtype=float), np.arange(S * N, dtype=float).reshape(S, N)]
WLEVELS = np.linspace(-1, 1, S * NWIN).reshape(S, 3, 3)

# method -> (host entry, bytes a slab stages, the call, where its argument list holds the inputs then the outputs: the positions
# behind the handle and the tracer, an array of pointers counting for all it holds)
_RING = ('contour_lengths', 'local_contour_lengths')         # the methods whose periodic form is another entry point
TWINS = {
    'contour_map': ('xc_contour_map', SLAB * 3, lambda c, p: c.contour_map(Q, LEVELS, VALUES), [6, 10, 12]),
    'coarsen': ('xc_coarsen', SLAB + 3 * 4 * 8, lambda c, p: c.coarsen(Q, 2, skipna=True), [8]),
    'contour_lengths': ('xc_contour_lengths', SLAB, lambda c, p: c.contour_lengths(Q, LEVELS, Y, X, radius=RADIUS, period=p),
                        lambda ring: [6, 7, 9 + ring, 12 + ring, 13 + ring]),
    'contour_lengths_scales': ('xc_contour_lengths_scales', SLAB,
                               lambda c, p: c.contour_lengths_scales(Q, LEVELS, Y, X, [2, 1], radius=RADIUS, period=p, skipna=True),
                               [6, 7, 13, 16, 17]),
    'contour_line_integrals': ('xc_contour_line_integrals', SLAB * 2,
                               lambda c, p: c.contour_line_integrals(Q, F, LEVELS, Y, X, radius=RADIUS, period=p), [3, 8, 9, 12, 15, 16, 17]),
    'local_contour_lengths': ('xc_local_contour_lengths', SLAB + 4 * NWIN * 8,
                              lambda c, p: c.local_contour_lengths(Q, Y, X, WIN, STR, 5, levels=WLEVELS, radius=RADIUS, period=p),
                              lambda ring: [6, 7] + [k + ring for k in (14, 15, 16, 17)]),
    'local_contour_lengths-window means': ('xc_local_contour_lengths', SLAB + 4 * NWIN * 8,
                                           lambda c, p: c.local_contour_lengths(Q, Y, X, WIN, STR, 5, radius=RADIUS, period=p),
                                           lambda ring: [6, 7] + [k + ring for k in (14, 15, 16, 17)]),
}
CASES = [(m, None) for m in TWINS] + [(m, PERIOD) for m in TWINS if m not in ('contour_map', 'coarsen')]


def _context(monkeypatch, names, cap):
    for name in names:                                              # where the entry point takes `nslab`: K15's integrand comes first
        monkeypatch.setitem(standin_lib._NSLAB_ARG, name, 5 if 'line_integrals' in name else 3)
    c = nat.Context.__new__(nat.Context)
    c.lib, c.handle, c.device = _Lib(), None, 0
    c._buffers, c._resident, c._staged, c._ev_pool = [], {}, [], []
    c.max_batch_bytes = cap
    return c


def _flat(v):
    """an argument as a list of its values: an array of pointers or ints as what it holds"""
    return list(v) if isinstance(v, C.Array) else [v]


@pytest.mark.parametrize('method,period', CASES, ids=['%s-%s' % (m, 'plain' if p is None else 'periodic') for m, p in CASES])
def test_the_dev_entry_gets_the_argument_list_of_the_host_entry(monkeypatch, method, period):
    host, slab_bytes, call, where = TWINS[method]
    if method.split('-')[0] in _RING and period is not None:
        host += '_periodic'
    if callable(where):
        where = where(0 if period is None else 1)
    runs = []
    for resident in (False, True):
        ctx = _context(monkeypatch, (host, host + '_dev'), 2 * slab_bytes + 8)
        if resident:
            ctx._resident[Q.ctypes.data] = Q
            ctx.lib.resident_base = Q.ctypes.data
        res = call(ctx, period)
        assert [c for c in ctx.lib.calls] == [(host + ('_dev' if resident else ''), n) for _, n in BATCHES]
        assert ctx._buffers == []
        runs.append((ctx.lib, [a for _, a in ctx.lib.args], res))
    (hlib, hargs, hres), (dlib, dargs, dres) = runs
    assert hlib.allocs == []                                        # the host form allocates nothing here
    allocs = iter(dlib.allocs)
    for ha, da, (s0, n) in zip(hargs, dargs, BATCHES):
        assert len(ha) == len(da)
        assert ha[1] == Q.ctypes.data + s0 * SLAB and da[1] == RES + s0 * SLAB
        mapped = [None, da[1]]
        for k in range(2, len(ha)):
            vals = _flat(ha[k])
            if k in where:
                for i, v in enumerate(vals):
                    if v is None:                                   # an absent optional input: no allocation, None in both lists
                        continue
                    assert not DEV <= v < RES                       # (a host pointer)
                    at, nbytes = next(allocs)
                    if at in dlib.mem:                              # an input: what went up is what the host entry would have read
                        assert dlib.mem[at] == C.string_at(v, nbytes)
                    vals[i] = at
            mapped.append(vals)
        assert mapped[2:] == [_flat(v) for v in da[2:]]
        assert all(type(h) is type(d) for h, d in zip(ha[2:], da[2:]))
    assert next(allocs, None) is None                               # every allocation is in an argument list, in order
    # the joined results have one container shape on both paths
    flat = lambda r: [r] if isinstance(r, np.ndarray) else list(r)
    assert type(hres) is type(dres)
    assert [(a.shape, a.dtype) for a in flat(hres)] == [(a.shape, a.dtype) for a in flat(dres)]


# what the device forms trust their caller with: refused by the binding under a mirror, in the host form's words, before anything
# reaches the library or is allocated
_DOWN = LEVELS[:, ::-1].copy()
_YINF = np.where(np.arange(NY) == 2, np.inf, Y)
_ASC, _FIN = '%s: contours must be ascending without NaN', '%s: coordinates must be finite'
TRUSTED = [
    ('xc_contour_lengths', nat.XC_EEDGES, _ASC, lambda c: c.contour_lengths(Q, _DOWN, Y, X)),
    ('xc_contour_lengths', nat.XC_EBADARG, _FIN, lambda c: c.contour_lengths(Q, LEVELS, _YINF, X)),
    ('xc_contour_lengths_scales', nat.XC_EEDGES, _ASC, lambda c: c.contour_lengths_scales(Q, _DOWN, Y, X, [2])),
    ('xc_contour_lengths_scales', nat.XC_EBADARG, _FIN, lambda c: c.contour_lengths_scales(Q, LEVELS, _YINF, X, [2])),
    ('xc_contour_line_integrals', nat.XC_EEDGES, _ASC, lambda c: c.contour_line_integrals(Q, F, _DOWN, Y, X)),
    ('xc_contour_line_integrals', nat.XC_EBADARG, _FIN, lambda c: c.contour_line_integrals(Q, F, LEVELS, _YINF, X)),
    ('xc_contour_map', nat.XC_EEDGES, 'non monotonic bins', lambda c: c.contour_map(Q, np.array([0.0, 1.0, 1.0, 2.0]), VALUES[:1])),
    ('xc_contour_map', nat.XC_EBADARG, '%s: the levels of every slab must be finite and strictly monotonic',
     lambda c: c.contour_map(Q, np.array([0.0, 2.0, 1.0, 3.0]), VALUES[:1])),
]


@pytest.mark.parametrize('who,code,text,call', TRUSTED, ids=['%s-%d' % (t[0], t[1]) for t in TRUSTED])
def test_under_a_mirror_the_binding_refuses_what_the_device_form_trusts(monkeypatch, who, code, text, call):
    ctx = _context(monkeypatch, (who, who + '_dev'), 8 << 30)
    ctx._resident[Q.ctypes.data] = Q
    ctx.lib.resident_base = Q.ctypes.data
    with pytest.raises(nat.XContourHipError) as e:
        call(ctx)
    assert e.value.code == code and str(e.value) == (text % who if '%s' in text else text)
    assert ctx.lib.calls == [] and ctx.lib.allocs == [] and ctx._buffers == []
