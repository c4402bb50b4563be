#!/usr/bin/env python3
"""K11 timing: xc_local_contour_lengths_dev on synthetic 3600 x 1801 float64 slabs made on the device (record_timing.synth_plane(ny,
nx, variant, nslab=slabs, host=False): variant 0 PV-like, 1 pure noise; no host copy), a `--window` x `--window` window every `--stride` nodes at the windows' means, lat / lon in radians.
Prints the event time per call; run it under `rocprofv3 --kernel-trace --stats -- python tools/local_clen_time.py ...` for the
per-kernel times.

    python tools/local_clen_time.py --slabs 1 --variant 0 --window 101 --stride 10 --reps 5
    python tools/local_clen_time.py --periodic             # windows run on round the longitude ring (xc_local_contour_lengths_periodic_dev)
"""
import argparse

import numpy as np

import record_timing as rt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--slabs', type=int, default=1)
    ap.add_argument('--variant', type=int, default=0)
    ap.add_argument('--window', type=int, default=101)
    ap.add_argument('--stride', type=int, default=10)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--ny', type=int, default=1801)
    ap.add_argument('--nx', type=int, default=3600)
    ap.add_argument('--periodic', action='store_true', help='periodic X: the period is 360 degrees (float32 radians)')
    ap.add_argument('--given', action='store_true', help='give the levels (the means of a first call): phase two alone')
    a = ap.parse_args()
    nat, ctx = rt.open_context()
    S, ny, nx, w, st = a.slabs, a.ny, a.nx, a.window, a.stride
    q, _, lat, lon, dlat, dlon = rt.synth_plane(ctx, nat, ny, nx, a.variant, nslab=S, host=False)
    y = np.deg2rad(lat.astype(np.float32)).astype(np.float64)
    x = np.deg2rad(lon.astype(np.float32)).astype(np.float64)
    dy, dx = ctx.to_device(y), ctx.to_device(x)
    nwin = -(-ny // st) * -(-nx // st)
    out, lvl, cnt = ctx.alloc(S * nwin * 8), ctx.alloc(S * nwin * 8), ctx.alloc(S * nwin * 8)
    given = ctx.alloc(S * nwin * 8)

    period = float(np.float64(np.deg2rad(np.float32(360.0))))

    def call(levels=None, lvl_out=lvl):
        if a.periodic:
            ctx._check(ctx.lib.xc_local_contour_lengths_periodic_dev(ctx.handle, q.ptr, nat.XC_F64, S, ny, nx, dy.ptr, dx.ptr, period,
                                                                     6371200.0, w, w, st, st, 1, levels, out.ptr, lvl_out.ptr, cnt.ptr))
        else:
            ctx._check(ctx.lib.xc_local_contour_lengths_dev(ctx.handle, q.ptr, nat.XC_F64, S, ny, nx, dy.ptr, dx.ptr, 6371200.0,
                                                            w, w, st, st, 1, levels, out.ptr, lvl_out.ptr, cnt.ptr))
    call(lvl_out=given)
    ctx.sync()
    levels = given.ptr if a.given else None
    call(levels)
    ctx.sync()
    e0, e1 = ctx.event(), ctx.event()
    ctx.record(e0)
    for _ in range(a.reps):
        call(levels)
    ctx.record(e1)
    ctx.sync()
    ms = ctx.elapsed_ms(e0, e1) / a.reps
    n = cnt.download((S, nwin), np.uint64)
    ln = out.download((S, nwin), np.float64)
    nodes = S * nwin * min(w, ny) * min(w, nx)
    print('slabs %d variant %d window %d stride %d%s%s: %d windows, %.1f us per call, %.2f us per slab, %.1f segments per window, '
          '%.1f %% of the windows with a contour, %.0f G window nodes per s'
          % (S, a.variant, w, st, ' periodic' if a.periodic else '', ' (levels given)' if a.given else '', S * nwin, ms * 1e3, ms * 1e3 / S, float(n.sum()) / (S * nwin),
             100.0 * float(np.mean(~np.isnan(ln))), nodes / (ms * 1e-3) / 1e9))


if __name__ == '__main__':
    main()
