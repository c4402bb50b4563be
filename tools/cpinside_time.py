#!/usr/bin/env python3
"""K18 timing: xc_contour_piece_interiors_dev on the inputs of tools/cpiece_time.py (one synthetic 1801 x 3600 float64 slab of
xc_synth_dev, variant 0: PV-like, 1: pure noise; N levels over the field's range; periodic X), beside K13 (xc_contour_pieces_dev) and
K17 (xc_contour_interior_dev, select 'all' and 'main', no mask) on the same device records.  The weight is cos(latitude) per node, the
integrand the field itself.  Every line is the mean of --reps calls from HIP events (xc_set_kernel_timing), the four stages of each
entry's own profile, and the wall clock around the synchronising call.

    python tools/cpinside_time.py --variant 0 --ncont 121 --reps 3
    python tools/cpinside_time.py --variant 1 --ncont 121 --reps 3
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
    ap.add_argument('--variant', type=int, default=0)
    ap.add_argument('--ncont', type=int, default=121)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--ny', type=int, default=1801)
    ap.add_argument('--nx', type=int, default=3600)
    a = ap.parse_args()
    from xcontour_amd import _native as nat
    ctx = nat.default_context(0)
    ny, nx, N = a.ny, a.nx, a.ncont
    lat = np.linspace(-90.0, 90.0, ny)
    lon = np.linspace(0.0, 360.0, nx, endpoint=False)
    dlat, dlon = ctx.to_device(lat), ctx.to_device(lon)
    q = ctx.alloc(ny * nx * 8)
    ctx._check(ctx.lib.xc_synth_dev(ctx.handle, q.ptr, nat.XC_F64, 1, ny, nx, dlat.ptr, dlon.ptr, 1, a.variant))
    qh = q.download((ny, nx), np.float64)
    mm = ctx.minmax(qh.reshape(1, -1))[0]
    lv = np.linspace(mm[0], mm[1], N)
    dw = ctx.to_device(np.ascontiguousarray(np.broadcast_to(np.cos(np.deg2rad(lat))[:, None], (ny, nx))))
    dc, dn, dpc = ctx.to_device(lv), ctx.alloc(N * 8), ctx.alloc(N * 8)
    head = (ctx.handle, q.ptr, nat.XC_F64, 1, ny, nx, dc.ptr, N, 0)
    f = ctx.lib.xc_contour_segments_periodic_dev
    rc = f(*head, 0, dn.ptr, None, None, None)
    if rc not in (0, 1):
        ctx._check(rc)
    total = int(dn.download((N,), np.uint64).sum())
    print('variant %d ncont %d periodic: %d segments' % (a.variant, N, total))
    df, dt, dp = ctx.alloc(max(total, 1) * 8), ctx.alloc(max(total, 1) * 8), ctx.alloc(max(total, 1) * 32)
    ctx._check(f(*head, total, dn.ptr, df.ptr, dt.ptr, dp.ptr))
    recs = (N, dn.ptr, df.ptr, dt.ptr, dp.ptr, ny, nx, 1)

    def report(name, call, profile, keys):
        call()
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            call()
        ctx.sync()
        wall = (time.perf_counter() - t0) / a.reps
        ctx.set_kernel_timing(True)
        call()
        acc = dict.fromkeys(keys, 0.0)
        for _ in range(a.reps):
            call()
            pr = profile()
            for k in keys:
                acc[k] += pr[k] / a.reps
        ctx.set_kernel_timing(False)
        print('%-22s wall %9.3f ms | %s | %d rounds, %d groups'
              % (name, wall * 1e3, ', '.join('%s %8.3f' % (k, acc[k]) for k in keys), pr['rounds'], pr['groups']))

    # K13
    k13 = (ctx.handle,) + recs + (dlat.ptr, dlon.ptr, 360.0, 0.0)
    rc = ctx.lib.xc_contour_pieces_dev(*k13, 0, dpc.ptr, *([None] * 8))
    if rc not in (0, 1):
        ctx._check(rc)
    npiece = int(dpc.download((N,), np.uint64).sum())
    rec = [ctx.alloc(max(npiece, 1) * 8) for _ in range(8)]
    report('K13 pieces', lambda: ctx._check(ctx.lib.xc_contour_pieces_dev(*k13, npiece, dpc.ptr, *[b.ptr for b in rec])),
           ctx.last_cpiece_profile, ('table_ms', 'rounds_ms', 'roots_ms', 'reduce_ms'))
    closed, wind = rec[2].download((npiece,), np.int32), rec[3].download((npiece,), np.int32)
    print('  %d pieces, %d rings, %d of them round the plane' % (npiece, int(closed.sum()), int((wind != 0).sum())))
    # K17
    out = [ctx.alloc(N * 8) for _ in range(3)]
    for name, sel in (('K17 interior all', 0), ('K17 interior main', 2)):
        report(name, lambda: ctx._check(ctx.lib.xc_contour_interior_dev(ctx.handle, *recs, sel, 0, N, dw.ptr, 0, q.ptr, nat.XC_F64, out[0].ptr,
                                                                        out[1].ptr, out[2].ptr, None)),
               ctx.last_cinterior_profile, ('table_ms', 'rounds_ms', 'select_ms', 'scan_ms'))
    # K18
    call = lambda: ctx._check(ctx.lib.xc_contour_piece_interiors_dev(ctx.handle, *recs, 0, N, dw.ptr, 0, q.ptr, nat.XC_F64, npiece, dpc.ptr,
                                                                     rec[0].ptr, rec[1].ptr, rec[2].ptr, rec[3].ptr, rec[4].ptr, rec[5].ptr,
                                                                     rec[6].ptr))
    report('K18 piece interiors', call, ctx.last_cpinside_profile, ('table_ms', 'rounds_ms', 'roots_ms', 'walk_ms'))
    n_in = rec[4].download((npiece,), np.int64)
    print('  %d nodes enclosed in all (the plane has %d), the largest interior %d' % (int(n_in[n_in > 0].sum()), ny * nx, int(n_in.max())))
    for b in [df, dt, dp, dc, dn, dpc, q, dlat, dlon, dw] + rec + out:
        b.free()


if __name__ == '__main__':
    main()
