#!/usr/bin/env python3
"""K19 timing: xc_contour_piece_tree_dev beside K18 (xc_contour_piece_interiors_dev) on the same device records:
one synthetic 1801 x 3600 float64 slab (record_timing.synth_plane(ny, nx, variant): variant 0 PV-like, 1 pure noise), N levels over
the field's range (levels_over), K12's periodic records of them (segment_records), the weight cos_weights(lat, ny, nx), the integrand the
field itself.  Every line is record_timing.report_means: the mean of --reps calls
after a warm-up: HIP events (xc_set_kernel_timing) for the stages of each entry's own profile, and the wall clock around the
synchronising call.  Then the shape of the tree: rings, rings with a parent, the largest depth, and the rows between the first edge of
every ring WITHOUT a parent and row 0 -- the steps of those rings' parent walks to within one row each (flip 0: the walks go up), a lower
bound of all parent walks.

    python tools/cptree_time.py --variant 0 --ncont 121 --reps 3
    python tools/cptree_time.py --variant 1 --ncont 121 --reps 3
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
    recs = (ctx.handle,) + seg.recs + (0, N, dw.ptr, 0, q.ptr, nat.XC_F64)
    report = functools.partial(rt.report_means, ctx, reps=a.reps)

    dpc = ctx.alloc(N * 8)
    npiece = rt.count_then(ctx, lambda: ctx.lib.xc_contour_piece_interiors_dev(*recs, 0, dpc.ptr, *([None] * 7)), dpc, N)
    rec = [ctx.alloc(max(npiece, 1) * 8) for _ in range(13)]
    k18 = [b.ptr for b in rec[:7]]
    w18, _ = report('K18 piece interiors', lambda: ctx._check(ctx.lib.xc_contour_piece_interiors_dev(*recs, npiece, dpc.ptr, *k18)),
                    ctx.last_cpinside_profile, ('table_ms', 'rounds_ms', 'roots_ms', 'walk_ms'))
    w19, _ = report('K19 piece tree', lambda: ctx._check(ctx.lib.xc_contour_piece_tree_dev(*recs, npiece, dpc.ptr, *[b.ptr for b in rec])),
                    ctx.last_cptree_profile, ('table_ms', 'rounds_ms', 'roots_ms', 'walk_ms', 'tree_ms'))
    print('  K19 / K18 wall: %.3f' % (w19 / w18))
    first, closed = rec[0].download((npiece,), np.int64), rec[2].download((npiece,), np.int32) != 0
    parent, depth = rec[7].download((npiece,), np.int64), rec[8].download((npiece,), np.int32)
    top = closed & (parent < 0)
    print('  %d pieces, %d rings, %d of them with a parent, largest depth %d' % (npiece, int(closed.sum()), int((parent >= 0).sum()),
                                                                                 int(depth.max()) if npiece else 0))
    print('  rings without a parent: %d, rows from their first edges to row 0: %d (mean %.1f)'
          % (int(top.sum()), int(((first[top] >> 1) // nx).sum()), float(((first[top] >> 1) // nx).mean()) if top.any() else 0.0))


if __name__ == '__main__':
    main()
