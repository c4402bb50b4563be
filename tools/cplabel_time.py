#!/usr/bin/env python3
"""K20 timing: xc_contour_piece_labels_dev beside K19 (xc_contour_piece_tree_dev) on the same device records -- the inputs of
tools/cptree_time.py (one synthetic 1801 x 3600 float64 slab of xc_synth_dev, variant 0: PV-like, 1: pure noise; N levels over the
field's range; periodic X; weight cos(latitude) per node, the integrand the field itself).  Every line is the mean of --reps calls
after a warm-up: HIP events (xc_set_kernel_timing) for the stages of each entry's own profile, and the wall clock around the
synchronising call.  Then the label scan (label_ms, the sixth stage of K20's profile) against the traffic it must move: per range
4 ny nx bytes of table entries, read in half-used lines, and 4 ny nx bytes of labels written; and the check that needs no reference:
bincount(label) == n_net for every ring.

    python tools/cplabel_time.py --variant 0 --ncont 121 --reps 3
    python tools/cplabel_time.py --variant 1 --ncont 121 --reps 3
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
    mm = ctx.minmax(q.download((ny, nx), np.float64).reshape(1, -1))[0]
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
    recs = (ctx.handle, N, dn.ptr, df.ptr, dt.ptr, dp.ptr, ny, nx, 1, 0, N, dw.ptr, 0, q.ptr, nat.XC_F64)

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
        print('%-22s wall %9.3f ms | %s | sum %8.3f | %d rounds, %d groups'
              % (name, wall * 1e3, ', '.join('%s %8.3f' % (k, acc[k]) for k in keys), sum(acc.values()), pr['rounds'], pr['groups']))
        return wall, acc

    rc = ctx.lib.xc_contour_piece_tree_dev(*recs, 0, dpc.ptr, *([None] * 13))
    if rc not in (0, 1):
        ctx._check(rc)
    npiece = int(dpc.download((N,), np.uint64).sum())
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
    for b in [df, dt, dp, dc, dn, dpc, q, dlat, dlon, dw, dlab] + rec:
        b.free()


if __name__ == '__main__':
    main()
