#!/usr/bin/env python3
"""The launch sequence of K13, K14, K16, K17 and K24 (the sibling of cprecords_trace.py, which does K18-K21): one call of
xc_contour_pieces_dev, xc_contour_polylines_dev, xc_contour_overturning_dev, xc_contour_interior_dev and xc_contour_folds_dev each, twice
(the first call warms up), on a 24 x 65 plane in three ranges of which the middle one has no segments (K12 traces two levels,
record_timing.segment_records; the empty range is put between them), periodic X ('main' selected) and
then plain ('all'), under a cap of ONE table row: two groups a call.  Then K22 (xc_label_overlap_dev on two block maps of the same three
ranges, the middle one without a ring: two groups under the same cap) and K23 (xc_ring_tracks_dev on 600 rings and 800 links), twice
each.  Meant to run under a kernel trace of its own (no counters):

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/cpiece_trace.py

The ordered (kernel, grid, block) lists of two builds of the library (XC_LIB_PATH names another one) are then compared line by line.
Prints the groups and rounds every call reports."""
import numpy as np

import record_timing as rt


def main():
    nat, ctx = rt.open_context()
    ny, nx, N = 24, 65, 3
    rng = np.random.default_rng(1)
    y, x = np.mgrid[0:ny, 0:nx]
    q = np.sin(2 * np.pi * x / nx) * np.cos(3 * np.pi * y / ny) + np.linspace(-1.0, 1.0, ny)[:, None] + 0.6 * rng.standard_normal((ny, nx))
    lv = np.array([-0.4, 0.5])
    dq, dc = ctx.to_device(q), ctx.to_device(lv)
    dw, df32 = ctx.to_device(rng.uniform(0.5, 1.5, (ny, nx))), ctx.to_device(rng.standard_normal((ny, nx)).astype(np.float32))
    dy, dx = ctx.to_device(np.arange(ny, dtype=np.float64)), ctx.to_device(np.arange(nx, dtype=np.float64))
    dpc = ctx.alloc(N * 8)
    ctx.set_cpiece_workspace(2 * ny * nx * 4)                                     # one row of the edge tables
    for periodic in (1, 0):
        seg = rt.segment_records(ctx, nat, dq, ny, nx, dc, 2, periodic)
        total = seg.total
        cnt = np.array([seg.counts[0, 0], 0, seg.counts[0, 1]], dtype=np.uint64)  # the records stay as they are: range 1 holds none
        dn = ctx.to_device(cnt)
        recs = (ctx.handle, N, dn.ptr, seg.df.ptr, seg.dt.ptr, seg.dp.ptr, ny, nx)
        out = [ctx.alloc(max(total * 32, N * ny * nx * 8)) for _ in range(15)]
        ptrs = [b.ptr for b in out]
        select = 2 if periodic else 0
        calls = (('pieces', 'cpiece', lambda: ctx.lib.xc_contour_pieces_dev(*recs, periodic, dy.ptr, dx.ptr, float(nx) if periodic else 0.0, 0.0,
                                                                            total, dpc.ptr, *ptrs)),
                 ('polylines', 'cjoin', lambda: ctx.lib.xc_contour_polylines_dev(*recs, total, dpc.ptr, *ptrs[:6])),
                 ('overturning', 'coverturn', lambda: ctx.lib.xc_contour_overturning_dev(*recs, periodic, select, *ptrs[:7])),
                 ('interior', 'cinterior', lambda: ctx.lib.xc_contour_interior_dev(*recs, periodic, select, 0, N, dw.ptr, 0, df32.ptr, nat.XC_F32,
                                                                                  *ptrs[:4])),
                 ('folds', 'cfold', lambda: ctx.lib.xc_contour_folds_dev(*recs, periodic, select, N, dw.ptr, 0, df32.ptr, nat.XC_F32, 1, *ptrs[:4],
                                                                         N * ((nx + 1) // 2), dpc.ptr, *ptrs[4:15])))
        for name, prof, call in calls:
            for _ in range(2):
                ctx._check(call())
            p = getattr(ctx, 'last_%s_profile' % prof)()
            print('periodic %d %-11s segments %s groups %d rounds %d' % (periodic, name, cnt.tolist(), p['groups'], p['rounds']))
        for b in [dn, seg.dn, seg.df, seg.dt, seg.dp] + out:                      # the plain pass starts from the memory the periodic one had
            b.free()
    # K22: blocks of 6 x 17 nodes against the same blocks shifted by (3, 5); range 1 holds no ring
    la = np.broadcast_to((y // 6) * 4 + x // 17, (N, ny, nx)).astype(np.int32)
    lb = np.broadcast_to(((y + 3) // 6) * 4 + (x + 5) // 17, (N, ny, nx)).astype(np.int32)
    la[1] = lb[1] = -1
    dla, dlb = ctx.to_device(la), ctx.to_device(lb)
    cap = 4096
    out = [ctx.alloc(cap * 8) for _ in range(5)]
    for _ in range(2):
        ctx._check(ctx.lib.xc_label_overlap_dev(ctx.handle, N, ny, nx, N, dla.ptr, dlb.ptr, dw.ptr, 0, df32.ptr, nat.XC_F32, cap, dpc.ptr,
                                                *[b.ptr for b in out]))
    print('overlap     pairs %s groups %d' % (dpc.download((N,), np.uint64).tolist(), ctx.last_cpoverlap_profile()['groups']))
    # K23: rings in steps of eight, links between the rings of consecutive steps
    nring, nlink = 600, 800
    a = rng.integers(0, nring - 8, nlink).astype(np.int64)
    graph = [ctx.to_device(v) for v in ((np.arange(nring) // 8).astype(np.int32), rng.integers(1, 50, nring).astype(np.int64), a,
                                        a + rng.integers(1, 9, nlink).astype(np.int64), rng.integers(0, 40, nlink).astype(np.int64))]
    rows = [ctx.alloc(nring * 8) for _ in range(11)]
    for _ in range(2):
        ctx._check(ctx.lib.xc_ring_tracks_dev(ctx.handle, nring, nlink, *[b.ptr for b in graph], 0.3, *[b.ptr for b in rows[:5]], nring, dpc.ptr,
                                              *[b.ptr for b in rows[5:]]))
    print('tracks      tracks %d rounds %d' % (int(dpc.download((1,), np.uint64)[0]), ctx.last_cptrack_profile()['rounds']))


if __name__ == '__main__':
    main()
