#!/usr/bin/env python3
"""K24 timing beside K17: xc_contour_folds_dev and xc_contour_interior_dev on the SAME device records, stage by stage from HIP events
(record_timing.stage_times with sync_each=True: this tool synchronises after every call).  Input: one synthetic 1801 x 3600 float64 slab
(synth_plane(ny, nx, variant): variant 0 PV-like; --ny / --nx resize it), or with --golden the barotropic field of tests/golden
(256 x 512); N levels over the field's range (levels_over); K12's periodic records (segment_records); select 'main' (or --select);
weights cos_weights(lat, ny, nx, offset=1e-3), the integrand the field itself.  Printed per stage: min / median / max over --reps warm
calls after one warm-up.
  K17  xc_contour_interior_dev with the integrand, no mask: table, rounds, select, scan
  K24  xc_contour_folds_dev, the sized call: table, rounds, select, columns (marks + column pass), runs, scan (fold scan + finish);
       the events found and the fold nodes touched
--root names another checkout of the package (its own library beside it; open_context(root)) to take the K17 numbers of that build; a build without K24
prints the K17 part only.

    python tools/cfold_time.py --ncont 121 --reps 5
    python tools/cfold_time.py --golden --ncont 121 --reps 5
"""
import argparse
import os

import numpy as np

import record_timing as rt
from record_timing import ROOT


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
    nat, ctx = rt.open_context(a.root)
    N = a.ncont
    sel = nat.Context.OVERTURN_SELECT[a.select]
    if a.golden:
        qh = np.load(os.path.join(ROOT, 'tests', 'golden', 'baro_q.npy')).astype(np.float64)
        ny, nx = qh.shape
        lat = np.load(os.path.join(ROOT, 'tests', 'golden', 'baro_lat.npy')).astype(np.float64)
        q = ctx.to_device(np.ascontiguousarray(qh))
    else:
        ny, nx = a.ny, a.nx
        q, qh, lat = rt.synth_plane(ctx, nat, ny, nx, a.variant)[:3]
    lv = rt.levels_over(ctx, qh, N)
    dw = ctx.to_device(rt.cos_weights(lat, ny, nx, offset=1e-3))
    seg = rt.segment_records(ctx, nat, q, ny, nx, ctx.to_device(lv), N, True)
    total = seg.total
    print('%s %d x %d, ncont %d periodic, select %s, gap %d: %d segments; min / median / max of %d warm calls, library of %s'
          % ('golden' if a.golden else 'variant %d' % a.variant, ny, nx, N, a.select, a.gap, total, a.reps, os.path.abspath(a.root)))

    def phases(call, profile, names):
        acc, pr = rt.stage_times(ctx, call, profile, names, a.reps, sync_each=True)
        for k in names:
            print('  %-10s %s' % (k[:-3], rt.min_med_max(acc[k], 1e3)))
        print('  rounds %d, groups %d' % (pr['rounds'], pr['groups']))
        return {k: [t * 1e3 for t in v] for k, v in acc.items()}

    # K17: with the integrand, no mask
    o17 = [ctx.alloc(N * 8) for _ in range(3)]
    k17 = lambda: ctx._check(ctx.lib.xc_contour_interior_dev(ctx.handle, *seg.recs, sel, 0, N, dw.ptr, 0, q.ptr, nat.XC_F64, o17[0].ptr, o17[1].ptr,
                                                             o17[2].ptr, None))
    print('K17 xc_contour_interior_dev (integrand, no mask)')
    a17 = phases(k17, ctx.last_cinterior_profile, ('table_ms', 'rounds_ms', 'select_ms', 'scan_ms'))
    print('  nodes scanned %d' % (N * ny * nx))
    if not hasattr(ctx, 'contour_folds'):
        print('K24: this build has none')
        return

    # K24: the count-only call sizes the event arrays of the timed one
    dense = [ctx.alloc(N * nx * b) for b in (4, 8, 8, 4)]
    dec = ctx.alloc(N * 8)
    head24 = (ctx.handle,) + seg.recs + (sel, N, dw.ptr, 0, q.ptr, nat.XC_F64, a.gap) + tuple(b.ptr for b in dense)
    ne = rt.count_then(ctx, lambda: ctx.lib.xc_contour_folds_dev(*head24, 0, dec.ptr, *([None] * 11)), dec, N)
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
