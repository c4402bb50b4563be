#!/usr/bin/env python3
"""K14 timing: the device join against the host join on one synthetic 1801 x 3600 float64 slab (record_timing.synth_plane(ny, nx,
variant): variant 0 PV-like, 1 pure noise; only its host copy is kept) and N levels over the field's range (levels_over).  One ROUTE per process, each after one untimed call:
  --route device   Context.contour_polylines: K12, K14 (xc_contour_polylines_dev), the download of the walk-ordered records and the
                   polyline table.  Then the stage times inside K14 from HIP events (record_timing.stage_times with warm=False: the
                   calls before it have warmed up; xc_last_cjoin_profile).
  --route host     the parent commit's route: Context.contour_segments (K12, the records to the host, sorted per range), then
                   join_segments (xc_join_segments, one thread); the two are timed apart.
  --route facade-device   Contour2D.trace_contours(levels, index=True, join='device', packed=True)
  --route facade-host     Contour2D.find_contours(levels, index=True): the parent's call (its untimed call is on a 64-row strip)
--periodic: the periodic forms.  Prints every repetition, so the spread is on the page.

    python tools/cjoin_time.py --route device --variant 0 --ncont 121 --reps 3
    python tools/cjoin_time.py --route host --variant 0 --ncont 121 --reps 1
"""
import argparse
import time

import numpy as np

import record_timing as rt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--route', choices=['device', 'host', 'facade-device', 'facade-host'], required=True)
    ap.add_argument('--variant', type=int, default=0)
    ap.add_argument('--ncont', type=int, default=121)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--ny', type=int, default=1801)
    ap.add_argument('--nx', type=int, default=3600)
    ap.add_argument('--periodic', action='store_true', help='periodic X: the seam cell column is traced too')
    a = ap.parse_args()
    nat, ctx = rt.open_context()
    import xcontour_amd as xa
    ny, nx, N = a.ny, a.nx, a.ncont
    q, qh, lat, lon, dlat, dlon = rt.synth_plane(ctx, nat, ny, nx, a.variant)
    for b in (q, dlat, dlon):                                                 # every route starts from the host array
        b.free()
    lv = rt.levels_over(ctx, qh, N)
    what = 'variant %d ncont %d%s' % (a.variant, N, ' periodic' if a.periodic else '')

    def facade(field, y):
        tr = xa.DataArray(field, ('latitude', 'longitude'), {'latitude': y, 'longitude': lon}, 'q')
        return xa.Contour2D(tr, np.ones(len(y)), {'X': 'longitude', 'Y': 'latitude'}, {'Y': 'latitude'}, dtype=np.float64)

    if a.route == 'device':
        ctx.contour_polylines(qh[None], lv, periodic=a.periodic)              # untimed
        for rep in range(a.reps):
            t0 = time.perf_counter()
            cnt, efw, ptw, poff, closed, rpo = ctx.contour_polylines(qh[None], lv, periodic=a.periodic)
            t = time.perf_counter() - t0
            print('%s device route rep %d: %.4f s  (%d segments, %d polylines, %d rings; %.1f MB downloaded)'
                  % (what, rep, t, efw.size, closed.size, int(closed.sum()), (efw.nbytes + ptw.nbytes + closed.size * 12) / 1e6))
        keys = ('table_ms', 'label_ms', 'rank_ms', 'place_ms', 'gather_ms')
        acc, pr = rt.stage_times(ctx, lambda: ctx.contour_polylines(qh[None], lv, periodic=a.periodic), ctx.last_cjoin_profile, keys, a.reps,
                                 sync_each=False, warm=False)
        for rep in range(a.reps):
            ms = [acc[k][rep] for k in keys]
            print('  K14 stages rep %d (ms): table %.3f, label rounds %.3f, roots + rank rounds %.3f, placement %.3f, gather %.3f; '
                  'sum %.3f; %d rounds over %d groups' % ((rep,) + tuple(ms) + (sum(ms), pr['rounds'], pr['groups'])))
    elif a.route == 'host':
        def route():
            t0 = time.perf_counter()
            cnt, ef, et, pts = ctx.contour_segments(qh[None], lv, periodic=a.periodic)
            t1 = time.perf_counter()
            off = np.concatenate([[0], np.cumsum(cnt.ravel().astype(np.int64))])
            walk, poff, closed, rpo = nat.join_segments(off, ef, et)
            t2 = time.perf_counter()
            return t1 - t0, t2 - t1, ef.size, closed.size
        route()                                                               # untimed
        for rep in range(a.reps):
            ts, tj, nseg, npoly = route()
            print('%s host route rep %d: contour_segments %.4f s, join_segments %.4f s, together %.4f s  (%d segments, %d polylines)'
                  % (what, rep, ts, tj, ts + tj, nseg, npoly))
    elif a.route == 'facade-device':
        cm = facade(qh, lat)
        kw = dict(index=True, periodic=a.periodic, join='device', packed=True)
        cm.trace_contours(lv, **kw)                                           # untimed
        for rep in range(a.reps):
            t0 = time.perf_counter()
            verts, voff, cl, wd, span = cm.trace_contours(lv, **kw)
            print('%s trace_contours(join=\'device\', packed=True) rep %d: %.4f s  (%d polylines, %d vertices)'
                  % (what, rep, time.perf_counter() - t0, cl.size, verts.shape[0]))
    else:
        facade(qh[:64], lat[:64]).find_contours(lv, index=True, periodic=a.periodic)      # untimed, on a strip
        cm = facade(qh, lat)
        for rep in range(a.reps):
            t0 = time.perf_counter()
            out = cm.find_contours(lv, index=True, periodic=a.periodic)
            print('%s find_contours (host join, nested) rep %d: %.4f s  (%d polylines)'
                  % (what, rep, time.perf_counter() - t0, sum(len(p) for p in out)))


if __name__ == '__main__':
    main()
