#!/usr/bin/env python3
"""K24 timing beside K17: xc_contour_folds_dev and xc_contour_interior_dev on the SAME device records, stage by stage from HIP events
(xc_set_kernel_timing).  Input: one synthetic 1801 x 3600 float64 slab of xc_synth_dev (variant 0: PV-like; --ny / --nx resize it), or
with --golden the barotropic field of tests/golden (256 x 512); N levels over the field's range; periodic X; select 'main' (or --select);
weights cos(latitude), the integrand the field itself.  Printed per stage: min / median / max over --reps warm calls after one warm-up.
  K17  xc_contour_interior_dev with the integrand, no mask: table, rounds, select, scan
  K24  xc_contour_folds_dev, the sized call: table, rounds, select, columns (marks + column pass), runs, scan (fold scan + finish);
       the events found and the fold nodes touched
--root names another checkout of the package (its own library beside it) to take the K17 numbers of that build; a build without K24
prints the K17 part only.

    python tools/cfold_time.py --ncont 121 --reps 5
    python tools/cfold_time.py --golden --ncont 121 --reps 5
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--variant', type=int, default=0)
    ap.add_argument('--ncont', type=int, default=121)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--ny', type=int, default=1801)
    ap.add_argument('--nx', type=int, default=3600)
    ap.add_argument('--gap', type=int, default=0)
    ap.add_argument('--golden', action='store_true', help='the barotropic field of tests/golden instead of the synthetic slab')
    ap.add_argument('--select', default='main', choices=['all', 'circumpolar', 'main'])
    ap.add_argument('--root', default=ROOT, help='the checkout whose package and library are timed')
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    from xcontour_amd import _native as nat
    ctx = nat.default_context(0)
    N = a.ncont
    sel = nat.Context.OVERTURN_SELECT[a.select]
    if a.golden:
        qh = np.load(os.path.join(ROOT, 'tests', 'golden', 'baro_q.npy')).astype(np.float64)
        ny, nx = qh.shape
        lat = np.load(os.path.join(ROOT, 'tests', 'golden', 'baro_lat.npy')).astype(np.float64)
        q = ctx.to_device(np.ascontiguousarray(qh))
    else:
        ny, nx = a.ny, a.nx
        lat = np.linspace(-90.0, 90.0, ny)
        lon = np.linspace(0.0, 360.0, nx, endpoint=False)
        dlat, dlon = ctx.to_device(lat), ctx.to_device(lon)
        q = ctx.alloc(ny * nx * 8)
        ctx._check(ctx.lib.xc_synth_dev(ctx.handle, q.ptr, nat.XC_F64, 1, ny, nx, dlat.ptr, dlon.ptr, 1, a.variant))
        qh = q.download((ny, nx), np.float64)
    mm = ctx.minmax(qh.reshape(1, -1))[0]
    lv = np.linspace(mm[0], mm[1], N)
    w = np.ascontiguousarray(np.broadcast_to(np.cos(np.deg2rad(lat))[:, None] + 1e-3, (ny, nx)))
    dw = ctx.to_device(w)
    dc, dn = ctx.to_device(lv), ctx.alloc(N * 8)
    head = (ctx.handle, q.ptr, nat.XC_F64, 1, ny, nx, dc.ptr, N, 0)
    f = ctx.lib.xc_contour_segments_periodic_dev
    rc = f(*head, 0, dn.ptr, None, None, None)
    if rc not in (0, 1):
        ctx._check(rc)
    total = int(dn.download((N,), np.uint64).sum())
    df, dt, dp = ctx.alloc(max(total, 1) * 8), ctx.alloc(max(total, 1) * 8), ctx.alloc(max(total, 1) * 32)
    ctx._check(f(*head, total, dn.ptr, df.ptr, dt.ptr, dp.ptr))
    print('%s %d x %d, ncont %d periodic, select %s, gap %d: %d segments; min / median / max of %d warm calls, library of %s'
          % ('golden' if a.golden else 'variant %d' % a.variant, ny, nx, N, a.select, a.gap, total, a.reps, os.path.abspath(a.root)))

    def phases(call, profile, names):
        ctx.set_kernel_timing(True)
        call()
        ctx.sync()
        acc = {k: [] for k in names}
        for _ in range(a.reps):
            call()
            ctx.sync()
            pr = profile()
            for k in names:
                acc[k].append(pr[k] * 1e3)
        ctx.set_kernel_timing(False)
        for k in names:
            v = acc[k]
            print('  %-10s %10.1f / %10.1f / %10.1f us' % (k[:-3], min(v), float(np.median(v)), max(v)))
        print('  rounds %d, groups %d' % (pr['rounds'], pr['groups']))
        return acc

    # K17: with the integrand, no mask
    o17 = [ctx.alloc(N * 8) for _ in range(3)]
    k17 = lambda: ctx._check(ctx.lib.xc_contour_interior_dev(ctx.handle, N, dn.ptr, df.ptr, dt.ptr, dp.ptr, ny, nx, 1, sel, 0, N, dw.ptr, 0,
                                                             q.ptr, nat.XC_F64, o17[0].ptr, o17[1].ptr, o17[2].ptr, None))
    print('K17 xc_contour_interior_dev (integrand, no mask)')
    a17 = phases(k17, ctx.last_cinterior_profile, ('table_ms', 'rounds_ms', 'select_ms', 'scan_ms'))
    print('  nodes scanned %d' % (N * ny * nx))
    if not hasattr(ctx, 'contour_folds'):
        print('K24: this build has none')
        return

    # K24: the count-only call sizes the event arrays of the timed one
    dense = [ctx.alloc(N * nx * b) for b in (4, 8, 8, 4)]
    dec = ctx.alloc(N * 8)
    head24 = (ctx.handle, N, dn.ptr, df.ptr, dt.ptr, dp.ptr, ny, nx, 1, sel, N, dw.ptr, 0, q.ptr, nat.XC_F64, a.gap) + tuple(b.ptr for b in dense)
    rc = ctx.lib.xc_contour_folds_dev(*head24, 0, dec.ptr, *([None] * 11))
    if rc not in (0, 1):
        ctx._check(rc)
    ne = int(dec.download((N,), np.uint64).sum())
    ev = [ctx.alloc(max(ne, 1) * b) for b in (4, 4, 4, 4, 8, 8, 16, 16, 16, 16, 16)]
    k24 = lambda: ctx._check(ctx.lib.xc_contour_folds_dev(*head24, ne, dec.ptr, *[b.ptr for b in ev]))
    print('K24 xc_contour_folds_dev (sized call)')
    a24 = phases(k24, ctx.last_cfold_profile, ('table_ms', 'rounds_ms', 'select_ms', 'columns_ms', 'runs_ms', 'scan_ms'))
    nodes = ev[6].download((ne, 2), np.int64) if ne else np.zeros((0, 2), dtype=np.int64)
    ncross = dense[0].download((N, nx), np.int32)
    print('  events %d, folded (level, column) pairs %d, fold nodes %d (under %d, over %d)'
          % (ne, int((ncross >= 3).sum()), int(nodes.sum()), int(nodes[:, 0].sum()), int(nodes[:, 1].sum())))
    m17, m24 = float(np.median(a17['scan_ms'])), float(np.median(a24['scan_ms']))
    print('fold scan + finish / K17 scan (medians): %.1f / %.1f us = %.3f; K17 scan spread %.1f us'
          % (m24, m17, m24 / m17 if m17 else float('nan'), max(a17['scan_ms']) - min(a17['scan_ms'])))


if __name__ == '__main__':
    main()
