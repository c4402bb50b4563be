#!/usr/bin/env python3
"""K15 and K10 timing: synthetic 3600 x 1801 float64 slabs made on the device (record_timing.synth_fill into one buffer, every variant
of --variants in turn: 0 PV-like, 1 pure noise), N levels from the range of slab 0 (levels_over), lat / lon in radians; the integrand
of K15 is a second synthetic slab (synth_fill with variant 0, seed=7).  Device events around `--reps` calls, `--rounds` times, K10 and K15 alternating; prints the
median and the range of the per-call times of each, one JSON line per variant.

    python tools/cline_time.py --variants 0 1 --ncont 121 --rounds 9
    python tools/cline_time.py --k10-only        # a library without K15 (XC_LIB_PATH: a diagnostic build of another K10)
"""
import argparse
import json
import os

import numpy as np

import record_timing as rt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--slabs', type=int, default=1)
    ap.add_argument('--variants', type=int, nargs='+', default=[0, 1])
    ap.add_argument('--ncont', type=int, default=121)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--ny', type=int, default=1801)
    ap.add_argument('--nx', type=int, default=3600)
    ap.add_argument('--k10-only', action='store_true')
    a = ap.parse_args()
    nat, ctx = rt.open_context()
    S, ny, nx, N = a.slabs, a.ny, a.nx, a.ncont
    lat, lon, dlat, dlon = rt.lat_lon(ctx, ny, nx)
    y = np.deg2rad(lat.astype(np.float32)).astype(np.float64)
    x = np.deg2rad(lon.astype(np.float32)).astype(np.float64)
    dy, dx = ctx.to_device(y), ctx.to_device(x)
    q, f = ctx.alloc(S * ny * nx * 8), ctx.alloc(S * ny * nx * 8)
    out = [ctx.alloc(S * N * 8) for _ in range(3)]
    for variant in a.variants:
        rt.synth_fill(ctx, nat, q, S, ny, nx, dlat, dlon, variant)
        rt.synth_fill(ctx, nat, f, S, ny, nx, dlat, dlon, 0, seed=7)
        dc = ctx.to_device(rt.levels_over(ctx, q.download((ny, nx), np.float64), N))

        def k10():
            ctx._check(ctx.lib.xc_contour_lengths_dev(ctx.handle, q.ptr, nat.XC_F64, S, ny, nx, dy.ptr, dx.ptr, 6371200.0,
                                                      dc.ptr, N, 0, out[1].ptr, out[2].ptr))

        def k15():
            ctx._check(ctx.lib.xc_contour_line_integrals_dev(ctx.handle, q.ptr, nat.XC_F64, f.ptr, nat.XC_F64, S, ny, nx, dy.ptr, dx.ptr,
                                                             0.0, 6371200.0, dc.ptr, N, 0, out[0].ptr, out[1].ptr, out[2].ptr))
        calls = {'K10': k10} if a.k10_only else {'K10': k10, 'K15': k15}
        e0, e1 = ctx.event(), ctx.event()
        times = {k: [] for k in calls}
        for k, fn in calls.items():                          # warm up: code objects, scratch
            fn()
        ctx.sync()
        for _ in range(a.rounds):
            for k, fn in calls.items():                      # alternating
                ctx.record(e0)
                for _ in range(a.reps):
                    fn()
                ctx.record(e1)
                ctx.sync()
                times[k].append(ctx.elapsed_ms(e0, e1) * 1e3 / a.reps)
        nseg = int(out[2].download((S, N), np.uint64).sum())
        rec = {'variant': variant, 'slabs': S, 'ncont': N, 'reps': a.reps, 'rounds': a.rounds, 'segments': nseg,
               'lib': os.path.basename(nat.LIB_PATH)}
        for k, t in times.items():
            rec[k + '_us'] = {'median': round(float(np.median(t)), 1), 'min': round(min(t), 1), 'max': round(max(t), 1)}
        if 'K15' in times:
            rec['K15_over_K10'] = round(float(np.median(times['K15']) / np.median(times['K10'])), 2)
        print(json.dumps(rec), flush=True)
        dc.free()                                            # the next variant's levels take its place


if __name__ == '__main__':
    main()
