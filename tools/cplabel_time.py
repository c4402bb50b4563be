#!/usr/bin/env python3
"""K20 timing: xc_contour_piece_labels_dev beside K19 (xc_contour_piece_tree_dev) on the same device records:
one synthetic 1801 x 3600 float64 slab (record_timing.synth_plane(ny, nx, variant): variant 0 PV-like, 1 pure noise), N levels over
the field's range (levels_over), K12's periodic records of them (segment_records), the weight cos_weights(lat, ny, nx), the integrand the
field itself.  Every line is record_timing.report_means: the mean of --reps calls
after a warm-up: HIP events (xc_set_kernel_timing) for the stages of each entry's own profile, and the wall clock around the
synchronising call.  Then the label scan (label_ms, the sixth stage of K20's profile) against the traffic it must move: per range
4 ny nx bytes of table entries, read in half-used lines, and 4 ny nx bytes of labels written; and the check that needs no reference:
bincount(label) == n_net for every ring.

    python tools/cplabel_time.py --variant 0 --ncont 121 --reps 3
    python tools/cplabel_time.py --variant 1 --ncont 121 --reps 3
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
    npiece = rt.count_then(ctx, lambda: ctx.lib.xc_contour_piece_tree_dev(*recs, 0, dpc.ptr, *([None] * 13)), dpc, N)
    rec = [ctx.alloc(max(npiece, 1) * 8) for _ in range(13)]
    dlab = ctx.alloc(N * ny * nx * 4)
    ptrs = [b.ptr for b in rec]
    keys = ('table_ms', 'rounds_ms', 'roots_ms', 'walk_ms', 'tree_ms')
    w19, _ = report('K19 piece tree', lambda: ctx._check(ctx.lib.xc_contour_piece_tree_dev(*recs, npiece, dpc.ptr, *ptrs)),
                    ctx.last_cptree_profile, keys)
    w20, acc = report('K20 piece labels', lambda: ctx._check(ctx.lib.xc_contour_piece_labels_dev(*recs, npiece, dpc.ptr, *ptrs, dlab.ptr)),
                      ctx.last_cplabel_profile, keys + ('label_ms',))
    print('  K20 / K19 wall: %.3f' % (w20 / w19))
    moved = 8.0 * N * ny * nx                                                  # 4 ny nx of table entries and 4 ny nx of labels per range
    print('  label scan: %.3f ms for %.3f GB that must move (table entries and labels): %.1f GB/s; the table is read twice (carry pass '
          'and scan) in half-used lines, so the lines fetched and stored are %.3f GB: %.1f GB/s'
          % (acc['label_ms'], moved / 1e9, moved / 1e6 / acc['label_ms'], 2.5 * moved / 1e9, 2.5 * moved / 1e6 / acc['label_ms']))
    pc = dpc.download((N,), np.uint64).astype(np.int64)
    closed, n_net = rec[2].download((npiece,), np.int32) != 0, rec[10].download((npiece,), np.int64)
    depth = rec[8].download((npiece,), np.int32)
    bad, inside, p0 = 0, 0, 0
    for k in range(N):                                                         # one level at a time: the map is 26 MB per level
        lab = dlab.download((ny * nx,), np.int32, offset_bytes=k * ny * nx * 4)
        cnt = np.bincount(lab[lab >= 0], minlength=int(pc[k]))
        sl = slice(p0, p0 + int(pc[k]))
        bad += int((cnt[closed[sl]] != n_net[sl][closed[sl]]).sum()) + int(cnt[~closed[sl]].sum()) + int(cnt.size != int(pc[k]))
        inside += int((lab >= 0).sum())
        p0 += int(pc[k])
    print('  %d pieces, %d rings, largest depth %d; %d of %d nodes lie in a ring; rings with bincount(label) != n_net: %d'
          % (npiece, int(closed.sum()), int(depth.max()) if npiece else 0, inside, N * ny * nx, bad))


if __name__ == '__main__':
    main()
