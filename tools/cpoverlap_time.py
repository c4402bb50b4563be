#!/usr/bin/env python3
"""K22 timing: xc_label_overlap_dev on the two maps of two K20 calls, beside K19, K20 and K21 on the same device records in one process
-- the inputs of tools/cpprops_time.py (one synthetic 1801 x 3600 float64 slab of xc_synth_dev, variant 0: PV-like, 1: pure noise; N
levels over the field's range; periodic X; weight cos(latitude) per node, the integrand the field itself).  Field B is field A rolled by
--roll columns.  Every line is the mean of --reps calls after a warm-up: HIP events (xc_set_kernel_timing) for the stages of each entry's
own profile, and the wall clock around the synchronising call.  Then the accumulate pass against the bytes it must read, the pairs
against the runs (on four levels, counted on the host from the downloaded maps: the load of the tables), and, for comparison only, the
host route K22 replaces on ONE level: downloading both maps, np.unique over the pairs and np.bincount for the three columns -- whose
rows are checked against K22's (n equal, the sums to 1e-9 of the sum of |terms|).

    python tools/cpoverlap_time.py --variant 0 --ncont 121 --reps 3
    python tools/cpoverlap_time.py --variant 1 --ncont 121 --reps 3
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
    ap.add_argument('--roll', type=int, default=5)
    a = ap.parse_args()
    from xcontour_amd import _native as nat
    ctx = nat.default_context(0)
    ny, nx, N = a.ny, a.nx, a.ncont
    lat = np.linspace(-90.0, 90.0, ny)
    lon = np.linspace(0.0, 360.0, nx, endpoint=False)
    dlat, dlon = ctx.to_device(lat), ctx.to_device(lon)
    qa = ctx.alloc(ny * nx * 8)
    ctx._check(ctx.lib.xc_synth_dev(ctx.handle, qa.ptr, nat.XC_F64, 1, ny, nx, dlat.ptr, dlon.ptr, 1, a.variant))
    qh = qa.download((ny, nx), np.float64)
    qb = ctx.to_device(np.ascontiguousarray(np.roll(qh, a.roll, axis=1)))
    mm = ctx.minmax(qh.reshape(1, -1))[0]
    lv = np.linspace(mm[0], mm[1], N)
    wh = np.ascontiguousarray(np.broadcast_to(np.cos(np.deg2rad(lat))[:, None], (ny, nx)))
    dw, dc = ctx.to_device(wh), ctx.to_device(lv)
    seg = ctx.lib.xc_contour_segments_periodic_dev
    fields = []
    for name, q in (('A', qa), ('B', qb)):
        dn, dpc = ctx.alloc(N * 8), ctx.alloc(N * 8)
        head = (ctx.handle, q.ptr, nat.XC_F64, 1, ny, nx, dc.ptr, N, 0)
        rc = seg(*head, 0, dn.ptr, None, None, None)
        if rc not in (0, 1):
            ctx._check(rc)
        total = int(dn.download((N,), np.uint64).sum())
        df, dt, dp = ctx.alloc(max(total, 1) * 8), ctx.alloc(max(total, 1) * 8), ctx.alloc(max(total, 1) * 32)
        ctx._check(seg(*head, total, dn.ptr, df.ptr, dt.ptr, dp.ptr))
        recs = (ctx.handle, N, dn.ptr, df.ptr, dt.ptr, dp.ptr, ny, nx, 1, 0, N, dw.ptr, 0, qa.ptr, nat.XC_F64)
        rc = ctx.lib.xc_contour_piece_tree_dev(*recs, 0, dpc.ptr, *([None] * 13))
        if rc not in (0, 1):
            ctx._check(rc)
        npiece = int(dpc.download((N,), np.uint64).sum())
        rec = [ctx.alloc(max(npiece, 1) * 8) for _ in range(13)]
        dlab = ctx.alloc(N * ny * nx * 4)
        print('variant %d ncont %d periodic, field %s: %d segments, %d pieces' % (a.variant, N, name, total, npiece))
        fields.append(dict(recs=recs, npiece=npiece, dpc=dpc, ptrs=[b.ptr for b in rec], dlab=dlab, keep=[dn, df, dt, dp, dpc] + rec))

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
    rc = ctx.lib.xc_label_overlap_dev(*head, 0, dpair.ptr, None, None, None, None, None)
    if rc not in (0, 1):
        ctx._check(rc)
    pairs = dpair.download((N,), np.uint64).astype(np.int64)
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
    for b in [qa, qb, dlat, dlon, dw, dc, dpair] + rows + dg + out + fa['keep'] + fb['keep'] + [fa['dlab'], fb['dlab']]:
        b.free()


if __name__ == '__main__':
    main()
