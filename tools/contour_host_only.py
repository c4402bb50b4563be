#!/usr/bin/env python3
"""The Python around the library calls of the contour family (K10 - K24), alone: `Context` methods and `Contour2D` methods of
K10 - K13 and of the record kernels K14, K16, K17, K19, K20, K24, K27 and K28 on a small stack (4 x 24 x 48 float32, 8 levels) against a stand-in
library whose entry points return at once.  No GPU needed; a sibling of tools/facade_host_only.py, which does the same for the Keff
sequence.  Every count download reads 2, so K12's, K13's and K24's second pass is staged too -- but zeros under find_contours, whose host
join wants real records (the join is the library's own xc_join_segments: build it first), and under the label rows, where a label
of 2 in a range of two pieces would point past the last range ("fill 0" in the row's name: the batch without segments, every label
-1 and no map fetched).  `--package DIR`: time the xcontour_amd package under DIR instead of this tree's (an A/B against another
revision's Python; point XC_LIB_PATH at a built library if DIR has none).  `--only WORD`: the rows whose name holds WORD.  Prints us per call, the best of `--rounds R` (default 5)
rounds of 400 calls.  On a shared host the figures drift by tens of percent from one process to the next whatever R: alternate the
two sides and compare medians and minima (profiles/contour_host_ab.md, profiles/ring_host_ab.md)."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[1:]
sys.path.insert(0, args[args.index('--package') + 1] if '--package' in args else ROOT)
import xcontour_amd as xa                 # noqa: E402
from xcontour_amd import _native as nat   # noqa: E402

NL, NY, NX, N = 4, 24, 48, 8
ROUNDS = int(args[args.index('--rounds') + 1]) if '--rounds' in args else 5


class _Lib(object):
    """every xc_* entry point returns XC_OK at once; a download reads `fill` in every uint64"""
    fill = 2
    _next = 1 << 40

    def __getattr__(self, name):
        if name == 'xc_malloc':
            return self._malloc
        if name == 'xc_memcpy_d2h':
            return self._d2h
        return lambda *a: 0

    def _malloc(self, h, n, pref):
        pref._obj.value = _Lib._next
        _Lib._next += (int(n) + 4095) & ~4095
        return 0

    def _d2h(self, h, dst, src, n):
        C.memset(dst, 0, n)
        if self.fill:
            (C.c_uint64 * (n // 8)).from_address(dst)[:] = [self.fill] * (n // 8)
        return 0


ctx = nat.Context.__new__(nat.Context)
ctx.lib, ctx.handle, ctx.device = _Lib(), None, 0
ctx._buffers, ctx._resident, ctx._staged, ctx._ev_pool = [], {}, [], []
ctx.max_batch_bytes = 8 << 30
nat.default_context = lambda device=0: ctx

rng = np.random.default_rng(0)
lat = np.linspace(-60, 60, NY).astype(np.float32); lon = (np.arange(NX) * 7.5).astype(np.float32); lev = np.arange(NL, dtype=np.float32)
q = rng.standard_normal((NL, NY, NX)).astype(np.float32)
tr = xa.DataArray(q, ('lev', 'lat', 'lon'), {'lev': lev, 'lat': lat, 'lon': lon}, 'pv')
cm = xa.Contour2D(tr, np.ones(NY), dims={'X': 'lon', 'Y': 'lat'}, dimEq={'Y': 'lat'}, increase=True, lt=True)
lv = np.linspace(-1.5, 1.5, N)
y, x = np.deg2rad(lat.astype(np.float64)), np.deg2rad(lon.astype(np.float64))
P = 2.0 * np.pi
wgt = np.ones((NY, NX))


def zeros(fn):
    def run():
        ctx.lib.fill = 0
        try:
            return fn()
        finally:
            ctx.lib.fill = 2
    return run


calls = [
    ('ctx.contour_lengths', lambda: ctx.contour_lengths(q, lv, y, x, radius=1.0, period=P)),
    ('ctx.local_contour_lengths', lambda: ctx.local_contour_lengths(q, y, x, (5, 5), (4, 4), 25, radius=1.0, period=P)),
    ('ctx.contour_segments', lambda: ctx.contour_segments(q, lv, periodic=True)),
    ('ctx.contour_pieces', lambda: ctx.contour_pieces(q, lv, y, x, radius=1.0, period=P)),
    ('cal_contour_lengths', lambda: cm.cal_contour_lengths(lv, latlon=True, periodic=True)),
    ('cal_local_contour_lengths', lambda: cm.cal_local_contour_lengths(5, stride=4, latlon=True, periodic=True)),
    ('find_contours', zeros(lambda: cm.find_contours(lv, periodic=True, return_closed=True))),
    ('cal_contour_pieces', lambda: cm.cal_contour_pieces(lv, latlon=True, periodic=True)),
    ('ctx.contour_polylines', lambda: ctx.contour_polylines(q, lv, periodic=True)),
    ('ctx.contour_overturning', lambda: ctx.contour_overturning(q, lv, periodic=True, select='main')),
    ('ctx.contour_interior', lambda: ctx.contour_interior(q, lv, w=wgt, f=q, periodic=True, select='main')),
    ('ctx.contour_piece_tree', lambda: ctx.contour_piece_tree(q, lv, w=wgt, f=q, periodic=True)),
    ('ctx.contour_piece_labels, fill 0', zeros(lambda: ctx.contour_piece_labels(q, lv, w=wgt, f=q, periodic=True))),
    ('cal_contour_piece_tree', lambda: cm.cal_contour_piece_tree(lv, integrand=tr, periodic=True)),
    ('cal_contour_piece_labels, fill 0', zeros(lambda: cm.cal_contour_piece_labels(lv, integrand=tr, periodic=True))),
    ('ctx.contour_folds', lambda: ctx.contour_folds(q, lv, w=wgt, f=q, periodic=True, select='main')),
    ('cal_contour_overturning', lambda: cm.cal_contour_overturning(lv, periodic=True)),
    ('cal_integral_inside_contours', lambda: cm.cal_integral_inside_contours(lv, integrand=tr, periodic=True)),
    ('cal_contour_folds', lambda: cm.cal_contour_folds(lv, integrand=tr, periodic=True)),
    ('ctx.contour_distance', lambda: ctx.contour_distance(q, lv, y, x, period=P, select='main', signed=True, return_nearest=True)),
    ('ctx.contour_distance_profile', lambda: ctx.contour_distance_profile(q, lv, y, x, [-2.0, -0.5, 0.5, 2.0], w=wgt, fields=(q, wgt), period=P,
                                                                          select='main', signed=True)),
]
if '--only' in args:                           # the rows whose name holds the word
    calls = [c for c in calls if args[args.index('--only') + 1] in c[0]]
tot = 0.0
with np.errstate(all='ignore'):                # (the stand-in leaves host-form outputs as np.empty made them)
    for name, fn in calls:
        for _ in range(20):
            fn()
        best = 1e9
        for _ in range(ROUNDS):
            t = time.perf_counter()
            for _ in range(400):
                fn()
            best = min(best, (time.perf_counter() - t) / 400 * 1e6)
        tot += best
        print('%-34s %7.1f us' % (name, best))
print('%-34s %7.1f us' % ('sum', tot))
