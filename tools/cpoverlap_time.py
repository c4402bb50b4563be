#!/usr/bin/env python3
"""K22 timing: xc_label_overlap_dev on the two maps of two K20 calls, beside K19, K20 and K21 on the same device records in one process:
field A is one synthetic 1801 x 3600 float64 slab (record_timing.synth_plane(ny, nx, variant): variant 0 PV-like, 1 pure noise), field B
is field A rolled by --roll columns; N levels over A's range (levels_over), K12's periodic records of each field (segment_records), the
weight cos_weights(lat, ny, nx), the integrand field A.  Every line is record_timing.report_means: the mean of --reps calls after a warm-up: HIP events (xc_set_kernel_timing) for the stages of each entry's
own profile, and the wall clock around the synchronising call.  Then the accumulate pass against the bytes it must read, the pairs
against the runs (on four levels, counted on the host from the downloaded maps: the load of the tables), and, for comparison only, the
host route K22 replaces on ONE level: downloading both maps, np.unique over the pairs and np.bincount for the three columns -- whose
rows are checked against K22's (n equal, the sums to 1e-9 of the sum of |terms|).

    python tools/cpoverlap_time.py --variant 0 --ncont 121 --reps 3
    python tools/cpoverlap_time.py --variant 1 --ncont 121 --reps 3
"""
import argparse
import functools
import time

import numpy as np

import record_timing as rt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--variant', type=int, default=0)
    ap.add_argument('--ncont', type=int, default=121)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--ny', type=int, default=1801)
    ap.add_argument('--nx', type=int, default=3600)
    ap.add_argument('--roll', type=int, default=5)
    a = ap.parse_args()
    nat, ctx = rt.open_context()
    ny, nx, N = a.ny, a.nx, a.ncont
    qa, qh, lat, lon, dlat, dlon = rt.synth_plane(ctx, nat, ny, nx, a.variant)
    qb = ctx.to_device(np.ascontiguousarray(np.roll(qh, a.roll, axis=1)))
    lv = rt.levels_over(ctx, qh, N)
    wh = rt.cos_weights(lat, ny, nx)
    dw, dc = ctx.to_device(wh), ctx.to_device(lv)
    fields = []
    for name, q in (('A', qa), ('B', qb)):
        seg = rt.segment_records(ctx, nat, q, ny, nx, dc, N, True)
        recs = (ctx.handle,) + seg.recs + (0, N, dw.ptr, 0, qa.ptr, nat.XC_F64)
        dpc = ctx.alloc(N * 8)
        npiece = rt.count_then(ctx, lambda: ctx.lib.xc_contour_piece_tree_dev(*recs, 0, dpc.ptr, *([None] * 13)), dpc, N)
        rec = [ctx.alloc(max(npiece, 1) * 8) for _ in range(13)]
        dlab = ctx.alloc(N * ny * nx * 4)
        print('variant %d ncont %d periodic, field %s: %d segments, %d pieces' % (a.variant, N, name, seg.total, npiece))
        fields.append(dict(recs=recs, npiece=npiece, dpc=dpc, ptrs=[b.ptr for b in rec], dlab=dlab))

    report = functools.partial(rt.report_means, ctx, reps=a.reps)
    keys = ('table_ms', 'rounds_ms', 'roots_ms', 'walk_ms', 'tree_ms')
    fa, fb = fields
    report('K19 piece tree A', lambda: ctx._check(ctx.lib.xc_contour_piece_tree_dev(*fa['recs'], fa['npiece'], fa['dpc'].ptr, *fa['ptrs'])),
           ctx.last_cptree_profile, keys)
    w20 = 0.0
    for name, fl in (('A', fa), ('B', fb)):
        w, _ = report('K20 piece labels %s' % name,
                      lambda: ctx._check(ctx.lib.xc_contour_piece_labels_dev(*fl['recs'], fl['npiece'], fl['dpc'].ptr, *fl['ptrs'], fl['dlab'].ptr)),
                      ctx.last_cplabel_profile, keys + ('label_ms',))
        w20 += w
    # K21 at nf = 3 (the three lat-lon moment planes) with the tracer as x: the figures of profiles/contour_piece_props.md
    la, lo = np.deg2rad(lat)[:, None], np.deg2rad(lon)[None, :]
    dg = [ctx.to_device(np.ascontiguousarray(p)) for p in (np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la) * np.ones_like(lo))]
    cap = max(fa['npiece'], 1)
    out = [ctx.alloc(3 * cap * 8), ctx.alloc(3 * cap * 8)] + [ctx.alloc(cap * 8) for _ in range(4)]
    gp = (nat._vp * 3)(*[b.ptr for b in dg])
    gd = (nat.C.c_int * 3)(*([nat.XC_F64] * 3))
    gs = (nat.C.c_int * 3)(0, 0, 0)
    more = (3, nat.C.cast(gp, nat._vp), nat.C.cast(gd, nat._vp), nat.C.cast(gs, nat._vp), qa.ptr, nat.XC_F64, *[b.ptr for b in out])
    report('K21 piece props nf 3', lambda: ctx._check(ctx.lib.xc_contour_piece_props_dev(*fa['recs'], fa['npiece'], fa['dpc'].ptr, *fa['ptrs'], *more)),
           ctx.last_cpprops_profile, keys + ('scan_ms', 'fold_ms'))

    # K22 on the two maps
    dpair = ctx.alloc(N * 8)
    head = (ctx.handle, N, ny, nx, N, fa['dlab'].ptr, fb['dlab'].ptr, dw.ptr, 0, qa.ptr, nat.XC_F64)
    pairs = rt.counts_then(ctx, lambda: ctx.lib.xc_label_overlap_dev(*head, 0, dpair.ptr, None, None, None, None, None), dpair, N).astype(np.int64)
    npair = int(pairs.sum())
    rows = [ctx.alloc(max(npair, 1) * b) for b in (4, 4, 8, 8, 8)]
    okeys = ('runs_ms', 'accumulate_ms', 'finish_ms')
    for name, h, last in (('K22 overlap w, f', head, rows[4].ptr), ('K22 overlap w', head[:-2] + (None, 0), None), ('K22 count only', head, None)):
        if name == 'K22 count only':
            call = lambda: ctx.lib.xc_label_overlap_dev(*h, 0, dpair.ptr, None, None, None, None, None)
        else:
            call = lambda: ctx._check(ctx.lib.xc_label_overlap_dev(*h, npair, dpair.ptr, *[b.ptr for b in rows[:4]], last))
        w22, acc = report(name, call, ctx.last_cpoverlap_profile, okeys)
        if name == 'K22 overlap w, f':
            must = N * ny * nx * (8.0 + 8.0 + 8.0)                              # two labels, w and f per node and range
            print('  K22 / (K20 A + K20 B) wall: %.3f' % (w22 / w20))
            print('  accumulate pass: %.3f ms for %.3f GB that must be read (two labels, w, f): %.1f GB/s'
                  % (acc['accumulate_ms'], must / 1e9, must / 1e6 / acc['accumulate_ms']))
    ctx._check(ctx.lib.xc_label_overlap_dev(*head, npair, dpair.ptr, *[b.ptr for b in rows]))   # w and f stand in the outputs
    print('  %d pairs in %d ranges (most in one range: %d)' % (npair, N, int(pairs.max())))

    # the load of the tables on four levels, and the host route on one of them
    rws = max(16, (ny + 31) // 32)
    off = np.concatenate([[0], np.cumsum(pairs)])
    for k in sorted(set([N // 8, N // 4, N // 2, (3 * N) // 4])):
        t0 = time.perf_counter()
        ma = fa['dlab'].download((ny, nx), np.int32, offset_bytes=k * ny * nx * 4)
        mb = fb['dlab'].download((ny, nx), np.int32, offset_bytes=k * ny * nx * 4)
        t1 = time.perf_counter()
        key = (ma.astype(np.int64) << 32) | (mb.astype(np.int64) & 0xffffffff)
        on = np.flatnonzero(key.ravel() != -1)
        uq, inv = np.unique(key.ravel()[on], return_inverse=True)
        n = np.bincount(inv, minlength=uq.size)
        sw = np.bincount(inv, weights=wh.ravel()[on], minlength=uq.size)
        swf = np.bincount(inv, weights=(wh * qh).ravel()[on], minlength=uq.size)
        t2 = time.perf_counter()
        start = np.ones((ny, nx), dtype=bool)
        start[1:] = key[1:] != key[:-1]
        start[::rws] = True
        runs = int((start & (key != -1)).sum())
        slots = 1 << max(2 * runs - 1, 1).bit_length() if runs else 0
        print('  level %3d: %7d pairs, %8d runs (chunks of %d rows), %9d slots: load %.4f | host route: download %.1f ms, unique + 3 bincount %.1f ms'
              % (k, uq.size, runs, rws, slots, uq.size / max(slots, 1), (t1 - t0) * 1e3, (t2 - t1) * 1e3))
        sl = slice(int(off[k]), int(off[k + 1]))
        g = [b.download((npair,), t)[sl] for b, t in zip(rows, (np.int32, np.int32, np.int64, np.float64, np.float64))]
        o = np.argsort((g[0].astype(np.int64) << 32) | (g[1].astype(np.int64) & 0xffffffff))
        sa = np.bincount(inv, weights=np.abs(wh * qh).ravel()[on], minlength=uq.size)
        bad = (uq.size != g[0].size) or int((g[2][o] != n).sum()) + int((np.abs(g[3][o] - sw) > 1e-9 * sw).sum()) \
            + int((np.abs(g[4][o] - swf) > 1e-9 * sa).sum())
        print('             rows that differ from the host route: %d' % int(bad))


if __name__ == '__main__':
    main()
