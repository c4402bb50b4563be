#!/usr/bin/env python3
"""The launch sequence of K18-K21: one call of xc_contour_piece_{interiors,tree,labels,props}_dev each, twice (the first call warms up),
on a 24 x 65 plane in three ranges of which the middle one has no segments (K12 traces two levels, record_timing.segment_records; the empty range is put
between them), periodic X and then plain, flip 0, with a weight, an integrand, three fields and x.  Meant to run under a kernel trace of its own (no counters):

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/cprecords_trace.py

Every call starts with its one k_ci_bound launch, so the trace splits into calls there; the ordered (kernel, grid, block) lists of two
builds of the library (XC_LIB_PATH names another one) are then compared line by line.  Prints the piece counts of every call."""
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
    dg = [ctx.to_device(rng.standard_normal((ny, nx))) for _ in range(3)]
    dpc = ctx.alloc(N * 8)
    for periodic in (1, 0):
        seg = rt.segment_records(ctx, nat, dq, ny, nx, dc, 2, periodic)
        total = seg.total
        cnt = np.array([seg.counts[0, 0], 0, seg.counts[0, 1]], dtype=np.uint64)  # the records stay as they are: range 1 holds none
        dn = ctx.to_device(cnt)
        recs = (ctx.handle, N, dn.ptr, seg.df.ptr, seg.dt.ptr, seg.dp.ptr, ny, nx, periodic, 0, N, dw.ptr, 0, df32.ptr, nat.XC_F32)
        rec = [ctx.alloc(total * 8) for _ in range(13)]
        ptrs = [b.ptr for b in rec]
        dlab = ctx.alloc(N * ny * nx * 4)
        out = [ctx.alloc(3 * total * 8), ctx.alloc(3 * total * 8)] + [ctx.alloc(total * 8) for _ in range(4)]
        gp = (nat._vp * 3)(*[b.ptr for b in dg])
        gd = (nat.C.c_int * 3)(*([nat.XC_F64] * 3))
        gs = (nat.C.c_int * 3)(0, 0, 0)
        more = (3, nat.C.cast(gp, nat._vp), nat.C.cast(gd, nat._vp), nat.C.cast(gs, nat._vp), dq.ptr, nat.XC_F64, *[b.ptr for b in out])
        calls = (('interiors', lambda: ctx.lib.xc_contour_piece_interiors_dev(*recs, total, dpc.ptr, *ptrs[:7])),
                 ('tree', lambda: ctx.lib.xc_contour_piece_tree_dev(*recs, total, dpc.ptr, *ptrs)),
                 ('labels', lambda: ctx.lib.xc_contour_piece_labels_dev(*recs, total, dpc.ptr, *ptrs, dlab.ptr)),
                 ('props', lambda: ctx.lib.xc_contour_piece_props_dev(*recs, total, dpc.ptr, *ptrs, *more)))
        for name, call in calls:
            for _ in range(2):
                ctx._check(call())
            print('periodic %d %-9s segments %s pieces %s' % (periodic, name, cnt.tolist(), dpc.download((N,), np.uint64).tolist()))
        for b in [dn, seg.dn, seg.df, seg.dt, seg.dp, dlab] + rec + out:           # the plain pass starts from the memory the periodic one had
            b.free()


if __name__ == '__main__':
    main()
