#!/usr/bin/env python3
"""K15 and K10 timing on the slabs of tools/clen_time.py: synthetic 3600 x 1801 float64 slabs made on the device (xc_synth_dev
variant 0: PV-like, 1: pure noise), N levels from the field's range, lat / lon in radians; the integrand of K15 is a second
synthetic slab (another seed).  Device events around `--reps` calls, `--rounds` times, K10 and K15 alternating; prints the
median and the range of the per-call times of each, one JSON line per variant.

    python tools/cline_time.py --variants 0 1 --ncont 121 --rounds 9
    python tools/cline_time.py --k10-only        # a library without K15 (XC_LIB_PATH: a diagnostic build of another K10)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    from xcontour_amd import _native as nat
    ctx = nat.Context(0)
    S, ny, nx, N = a.slabs, a.ny, a.nx, a.ncont
    lat = np.linspace(-90.0, 90.0, ny)
    lon = np.linspace(0.0, 360.0, nx, endpoint=False)
    dlat, dlon = ctx.to_device(lat), ctx.to_device(lon)
    y = np.deg2rad(lat.astype(np.float32)).astype(np.float64)
    x = np.deg2rad(lon.astype(np.float32)).astype(np.float64)
    dy, dx = ctx.to_device(y), ctx.to_device(x)
    q, f = ctx.alloc(S * ny * nx * 8), ctx.alloc(S * ny * nx * 8)
    out = [ctx.alloc(S * N * 8) for _ in range(3)]
    for variant in a.variants:
        ctx._check(ctx.lib.xc_synth_dev(ctx.handle, q.ptr, nat.XC_F64, S, ny, nx, dlat.ptr, dlon.ptr, 1, variant))
        ctx._check(ctx.lib.xc_synth_dev(ctx.handle, f.ptr, nat.XC_F64, S, ny, nx, dlat.ptr, dlon.ptr, 7, 0))
        mm = ctx.minmax(q.download((1, ny * nx), np.float64))[0]
        dc = ctx.to_device(np.linspace(mm[0], mm[1], N))

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
        dc.free()
    ctx.close()


if __name__ == '__main__':
    main()
