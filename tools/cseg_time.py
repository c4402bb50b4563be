#!/usr/bin/env python3
"""K12 timing: xc_contour_segments_dev on the synthetic 3600 x 1801 float64 slabs of tools/clen_time.py (xc_synth_dev variant 0:
PV-like, 1: pure noise), N levels from the field's range.  Reports, per call,
  count   the count-only call (capacity 0): count pass + the two scan kernels + the one read-back of the total;
  full    the call into exactly sized buffers: the above + the emit pass (emit = full - count);
  join    xc_join_segments on the host, records already downloaded (skipped above --join-max segments);
  facade  Contour2D.find_contours(levels, index=True) on the same slab, host arrays in, polylines out (skipped likewise).
Wall-clock times around calls that end in a stream synchronisation.  --periodic: the periodic forms
(xc_contour_segments_periodic_dev, find_contours(periodic=True)): the ring of nx cell columns.

    python tools/cseg_time.py --variant 0 --ncont 121 --reps 5
    python tools/cseg_time.py --variant 0 --ncont 121 --reps 5 --periodic
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--slabs', type=int, default=1)
    ap.add_argument('--variant', type=int, default=0)
    ap.add_argument('--ncont', type=int, default=121)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--ny', type=int, default=1801)
    ap.add_argument('--nx', type=int, default=3600)
    ap.add_argument('--periodic', action='store_true', help='periodic X: the seam cell column is traced too')
    ap.add_argument('--join-max', type=int, default=30000000, help='most segments the host join and the facade call are timed on')
    a = ap.parse_args()
    import xcontour_amd as xa
    from xcontour_amd import _native as nat
    ctx = nat.default_context(0)
    S, ny, nx, N = a.slabs, a.ny, a.nx, a.ncont
    lat = np.linspace(-90.0, 90.0, ny)
    lon = np.linspace(0.0, 360.0, nx, endpoint=False)
    dlat, dlon = ctx.to_device(lat), ctx.to_device(lon)
    q = ctx.alloc(S * ny * nx * 8)
    ctx._check(ctx.lib.xc_synth_dev(ctx.handle, q.ptr, nat.XC_F64, S, ny, nx, dlat.ptr, dlon.ptr, 1, a.variant))
    mm = ctx.minmax(q.download((1, ny * nx), np.float64))[0]
    lv = np.linspace(mm[0], mm[1], N)
    dc, dn = ctx.to_device(lv), ctx.alloc(S * N * 8)
    head = (ctx.handle, q.ptr, nat.XC_F64, S, ny, nx, dc.ptr, N, 0)
    f = ctx.lib.xc_contour_segments_periodic_dev if a.periodic else ctx.lib.xc_contour_segments_dev

    def timed(fn):
        fn()
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        ctx.sync()
        return (time.perf_counter() - t0) / a.reps

    def count():
        rc = f(*head, 0, dn.ptr, None, None, None)
        if rc not in (0, 1):
            ctx._check(rc)
    t_count = timed(count)
    cnt = dn.download((S, N), np.uint64)
    total = int(cnt.sum())
    cells = S * (ny - 1) * (nx if a.periodic else nx - 1)
    print('slabs %d variant %d ncont %d%s: %d segments (%.2f per cell, %.1f MB of records)'
          % (S, a.variant, N, ' periodic' if a.periodic else '', total, total / cells, total * 48 / 1e6))
    print('count pass  %10.1f us per call' % (t_count * 1e6))
    df, dt, dp = ctx.alloc(max(total, 1) * 8), ctx.alloc(max(total, 1) * 8), ctx.alloc(max(total, 1) * 32)
    t_full = timed(lambda: ctx._check(f(*head, total, dn.ptr, df.ptr, dt.ptr, dp.ptr)))
    print('count+emit  %10.1f us per call  (emit pass %.1f us, %.0f GB/s of records)'
          % (t_full * 1e6, (t_full - t_count) * 1e6, total * 48 / max(t_full - t_count, 1e-9) / 1e9))
    if total <= a.join_max:
        ef, et = df.download((total,), np.int64), dt.download((total,), np.int64)
        off = np.concatenate([[0], np.cumsum(cnt.ravel().astype(np.int64))])
        t0 = time.perf_counter()
        _, poff, closed, _ = nat.join_segments(off, ef, et)
        print('host join   %10.1f us  (%d polylines, %d of them rings)' % ((time.perf_counter() - t0) * 1e6, closed.size, int(closed.sum())))
        qh = q.download((ny, nx), np.float64)
        tr = xa.DataArray(qh, ('latitude', 'longitude'), {'latitude': lat, 'longitude': lon}, 'q')
        cm = xa.Contour2D(tr, np.ones(ny), {'X': 'longitude', 'Y': 'latitude'}, {'Y': 'latitude'}, dtype=np.float64)
        cm.find_contours(lv[:2], index=True, periodic=a.periodic)
        t0 = time.perf_counter()
        out = cm.find_contours(lv, index=True, periodic=a.periodic)
        print('facade      %10.1f us  (find_contours of slab 0, %d polylines kept)' % ((time.perf_counter() - t0) * 1e6, sum(len(p) for p in out)))
    else:
        print('host join   not measured (more than --join-max segments)')
        print('facade      not measured (more than --join-max segments)')
    for b in (df, dt, dp, dc, dn, q, dlat, dlon):
        b.free()


if __name__ == '__main__':
    main()
