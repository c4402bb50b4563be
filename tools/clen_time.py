#!/usr/bin/env python3
"""K10 timing: xc_contour_lengths_dev on synthetic 3600 x 1801 float64 slabs made on the device (record_timing.synth_plane(ny, nx,
variant, nslab=slabs): variant 0 PV-like, 1 pure noise), N levels from the range of slab 0 (levels_over), lat / lon in radians.  Prints the event time per call; run it under
`rocprofv3 --kernel-trace --stats -- python tools/clen_time.py ...` for the per-kernel times.

    python tools/clen_time.py --slabs 64 --variant 0 --ncont 121 --reps 5
    python tools/clen_time.py --slabs 64 --periodic        # the longitude ring closed (xc_contour_lengths_periodic_dev)
"""
import argparse

import numpy as np

import record_timing as rt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--slabs', type=int, default=1)
    ap.add_argument('--variant', type=int, default=0)
    ap.add_argument('--ncont', type=int, default=121)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--ny', type=int, default=1801)
    ap.add_argument('--nx', type=int, default=3600)
    ap.add_argument('--periodic', action='store_true', help='periodic X: the period is 360 degrees (float32 radians)')
    a = ap.parse_args()
    nat, ctx = rt.open_context()
    S, ny, nx = a.slabs, a.ny, a.nx
    q, qh, lat, lon, dlat, dlon = rt.synth_plane(ctx, nat, ny, nx, a.variant, nslab=S)
    lv = rt.levels_over(ctx, qh, a.ncont)
    y = np.deg2rad(lat.astype(np.float32)).astype(np.float64)
    x = np.deg2rad(lon.astype(np.float32)).astype(np.float64)
    dy, dx, dc = ctx.to_device(y), ctx.to_device(x), ctx.to_device(lv)
    out, cnt = ctx.alloc(S * a.ncont * 8), ctx.alloc(S * a.ncont * 8)

    period = float(np.float64(np.deg2rad(np.float32(360.0))))

    def call():
        if a.periodic:
            ctx._check(ctx.lib.xc_contour_lengths_periodic_dev(ctx.handle, q.ptr, nat.XC_F64, S, ny, nx, dy.ptr, dx.ptr, period, 6371200.0,
                                                               dc.ptr, a.ncont, 0, out.ptr, cnt.ptr))
        else:
            ctx._check(ctx.lib.xc_contour_lengths_dev(ctx.handle, q.ptr, nat.XC_F64, S, ny, nx, dy.ptr, dx.ptr, 6371200.0,
                                                      dc.ptr, a.ncont, 0, out.ptr, cnt.ptr))
    call()
    ctx.sync()
    e0, e1 = ctx.event(), ctx.event()
    ctx.record(e0)
    for _ in range(a.reps):
        call()
    ctx.record(e1)
    ctx.sync()
    ms = ctx.elapsed_ms(e0, e1) / a.reps
    n = cnt.download((S, a.ncont), np.uint64)
    cells = S * (ny - 1) * (nx if a.periodic else nx - 1)
    print('slabs %d variant %d ncont %d%s: %.1f us per call, %.2f us per slab, %.2f segments per cell, %.0f GB/s of tracer'
          % (S, a.variant, a.ncont, ' periodic' if a.periodic else '', ms * 1e3, ms * 1e3 / S, float(n.sum()) / cells, S * ny * nx * 8 / (ms * 1e-3) / 1e9))


if __name__ == '__main__':
    main()
