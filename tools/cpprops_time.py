#!/usr/bin/env python3
"""K21 timing: xc_contour_piece_props_dev beside K19 (xc_contour_piece_tree_dev) and K20 (xc_contour_piece_labels_dev) on the same device
records in one process: one synthetic 1801 x 3600 float64 slab (record_timing.synth_plane(ny, nx, variant): variant 0 PV-like, 1 pure
noise), N levels over the field's range (levels_over), K12's periodic records of them (segment_records), the weight
cos_weights(lat, ny, nx), the integrand the field itself.  K21 runs at nf = 3 (the three lat-lon moment planes, shared float64 planes)
with the tracer as x, and at nf = 8 (those and five per-slab float64 stacks) with the tracer as x.  Every line is
record_timing.report_means: the mean of --reps calls after a warm-up: HIP events (xc_set_kernel_timing) for the stages of each entry's
own profile, and the wall clock around the synchronising call.  Then the props scan (scan_ms) against the bytes it must read,
and the checks against K20's map that need no reference: per ring the minimum and maximum of x over its label and the smallest flat node
of the minimum (exact), and the first field's net sum against np.bincount(label, weights) (to 1e-9 of the sum of |terms|).

    python tools/cpprops_time.py --variant 0 --ncont 121 --reps 3
    python tools/cpprops_time.py --variant 1 --ncont 121 --reps 3
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
    cap = max(npiece, 1)
    rec = [ctx.alloc(cap * 8) for _ in range(13)]
    dlab = ctx.alloc(N * ny * nx * 4)
    ptrs = [b.ptr for b in rec]
    keys = ('table_ms', 'rounds_ms', 'roots_ms', 'walk_ms', 'tree_ms')
    w19, _ = report('K19 piece tree', lambda: ctx._check(ctx.lib.xc_contour_piece_tree_dev(*recs, npiece, dpc.ptr, *ptrs)),
                    ctx.last_cptree_profile, keys)
    w20, _ = report('K20 piece labels', lambda: ctx._check(ctx.lib.xc_contour_piece_labels_dev(*recs, npiece, dpc.ptr, *ptrs, dlab.ptr)),
                    ctx.last_cplabel_profile, keys + ('label_ms',))
    fe20 = rec[0].download((npiece,), np.int64)                               # the order of the rows inside a range is the call's own
    # the fields: three shared moment planes, five per-slab stacks
    la, lo = np.deg2rad(lat)[:, None], np.deg2rad(lon)[None, :]
    shared = [np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la) * np.ones_like(lo)]
    dg = [ctx.to_device(np.ascontiguousarray(p)) for p in shared] + [ctx.to_device(np.ascontiguousarray(qh * (k + 2.0))) for k in range(5)]
    out = [ctx.alloc(8 * cap * 8), ctx.alloc(8 * cap * 8)] + [ctx.alloc(cap * 8) for _ in range(4)]
    walls = {}
    for nf in (3, 8):
        gp = (nat._vp * 8)(*[b.ptr for b in dg])
        gd = (nat.C.c_int * 8)(*([nat.XC_F64] * 8))
        gs = (nat.C.c_int * 8)(*([0] * 3 + [1] * 5))
        more = (nf, nat.C.cast(gp, nat._vp), nat.C.cast(gd, nat._vp), nat.C.cast(gs, nat._vp), q.ptr, nat.XC_F64, *[b.ptr for b in out])
        w21, acc = report('K21 piece props nf %d' % nf, lambda: ctx._check(ctx.lib.xc_contour_piece_props_dev(*recs, npiece, dpc.ptr, *ptrs, *more)),
                          ctx.last_cpprops_profile, keys + ('scan_ms', 'fold_ms'))
        walls[nf] = w21
        print('  K21 / K19 wall: %.3f   K21 / K20 wall: %.3f' % (w21 / w19, w21 / w20))
        passes = 2                                                             # fields in runs of four; the places of x ride on the second pass
        must = N * ny * nx * (4.0 + 8.0 * max(nf - 3, 0) + 8.0)                # table + per-slab f64 fields + x, per range
        print('  props scan: %.3f ms (%d passes and the carry pass) for %.3f GB that must be read (table entries, per-slab fields, x): %.1f GB/s'
              % (acc['scan_ms'], passes, must / 1e9, must / 1e6 / acc['scan_ms']))
    # nf = 8 stands in the outputs: against K20's map
    pc = dpc.download((N,), np.uint64).astype(np.int64)
    closed = rec[2].download((npiece,), np.int32) != 0
    fe21 = rec[0].download((npiece,), np.int64)
    net0 = out[0].download((npiece,), np.float64)
    xmin, xmax = out[2].download((npiece,), np.float64), out[3].download((npiece,), np.float64)
    amin = out[4].download((npiece,), np.int64)
    wq = (np.cos(la) * np.ones_like(lo) * shared[0]).ravel()
    xq = qh.ravel()
    bad_x, bad_at, bad_sum, p0 = 0, 0, 0, 0
    for k in range(N):                                                         # one level at a time: the map is 26 MB per level
        lab = dlab.download((ny * nx,), np.int32, offset_bytes=k * ny * nx * 4)
        n = int(pc[k])
        sl = slice(p0, p0 + n)
        p0 += n
        if n == 0:
            continue
        to21 = np.empty(n, dtype=np.int64)                                    # K20's row -> K21's row: both sorted by first_edge
        to21[np.argsort(fe20[sl])] = np.argsort(fe21[sl])
        on = np.flatnonzero(lab >= 0)
        lab = np.where(lab >= 0, to21[np.maximum(lab, 0)], -1)
        lo_, hi_ = np.full(n, np.inf), np.full(n, -np.inf)
        np.minimum.at(lo_, lab[on], xq[on])
        np.maximum.at(hi_, lab[on], xq[on])
        cl = closed[sl] & np.isfinite(lo_)
        bad_x += int((lo_[cl] != xmin[sl][cl]).sum()) + int((hi_[cl] != xmax[sl][cl]).sum())
        hit = on[xq[on] == lo_[lab[on]]]                                       # the nodes that carry their ring's minimum, ascending
        first = np.full(n, -1, dtype=np.int64)
        first[lab[hit][::-1]] = hit[::-1]
        bad_at += int((first[cl] != amin[sl][cl]).sum())
        s = np.bincount(lab[on], weights=wq[on], minlength=n)
        sa = np.bincount(lab[on], weights=np.abs(wq[on]), minlength=n)
        bad_sum += int((np.abs(s - net0[sl])[cl] > 1e-9 * sa[cl]).sum())
    print('  %d pieces, %d rings; rings whose extremum of x differs from the map\'s: %d; whose place of the minimum differs: %d; '
          'whose first net sum differs from bincount by more than 1e-9: %d' % (npiece, int(closed.sum()), bad_x, bad_at, bad_sum))


if __name__ == '__main__':
    main()
