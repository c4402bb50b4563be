#!/usr/bin/env python3
"""K18 timing: xc_contour_piece_interiors_dev beside K13 (xc_contour_pieces_dev) and K17 (xc_contour_interior_dev, select 'all' and 'main',
no mask) on the same device records: one synthetic 1801 x 3600 float64 slab (record_timing.synth_plane(ny, nx, variant): variant 0 PV-like, 1 pure noise), N levels over
the field's range (levels_over), K12's periodic records of them (segment_records), the weight cos_weights(lat, ny, nx), the integrand the
field itself.  Every line is record_timing.report_means(with_sum=False): the mean of --reps calls from HIP
events (xc_set_kernel_timing), the four stages of each entry's own profile, and the wall clock around the synchronising call.

    python tools/cpinside_time.py --variant 0 --ncont 121 --reps 3
    python tools/cpinside_time.py --variant 1 --ncont 121 --reps 3
"""
import argparse
import functools

import numpy as np

import record_timing as rt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--variant', type=int, default=0)
    ap.add_argument('--ncont', type=int, default=121)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--ny', type=int, default=1801)
    ap.add_argument('--nx', type=int, default=3600)
    a = ap.parse_args()
    nat, ctx = rt.open_context()
    ny, nx, N = a.ny, a.nx, a.ncont
    q, qh, lat, lon, dlat, dlon = rt.synth_plane(ctx, nat, ny, nx, a.variant)
    lv = rt.levels_over(ctx, qh, N)
    dw = ctx.to_device(rt.cos_weights(lat, ny, nx))
    seg = rt.segment_records(ctx, nat, q, ny, nx, ctx.to_device(lv), N, True)
    print('variant %d ncont %d periodic: %d segments' % (a.variant, N, seg.total))
    recs = seg.recs
    report = functools.partial(rt.report_means, ctx, reps=a.reps, with_sum=False)

    # K13
    k13 = (ctx.handle,) + recs + (dlat.ptr, dlon.ptr, 360.0, 0.0)
    dpc = ctx.alloc(N * 8)
    npiece = rt.count_then(ctx, lambda: ctx.lib.xc_contour_pieces_dev(*k13, 0, dpc.ptr, *([None] * 8)), dpc, N)
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


if __name__ == '__main__':
    main()
