#!/usr/bin/env python3
"""K16 timing: xc_contour_overturning_dev on one synthetic 1801 x 3600 float64 slab (record_timing.synth_plane(ny, nx, variant):
variant 0 PV-like, 1 pure noise), N levels over the field's range (levels_over) and K12's periodic records of them (SegmentRecords).  In
ONE run, on the same records:
  K12      xc_contour_segments_periodic_dev into exactly sized device buffers (count + emit), wall clock;
  K16      xc_contour_overturning_dev (select 'main', or --select), wall clock, and inside it from HIP events (xc_set_kernel_timing):
           table     clearing the edge tables, scatter, link, and handing the tables on clean
           rounds    the pointer-doubling rounds
           select    roots, per-piece sums, the pick of the main ring
           count     the count pass with the init and finish passes over the dense outputs
  K13      xc_contour_pieces_dev, which shares Phase A, the same way (its phases: table, rounds, roots, reduce);
  facade   Context.contour_overturning and Context.contour_pieces from a host array (upload, K12 twice, the call, download);
with --user (variant 0 is what it is meant for) the route a user had before K16: trace_contours(join='device', packed=True,
index=True) and a numpy count over its vertices (np.add.at on the vertices that lie on a grid line along Y).
Every wall time is the minimum / median / maximum over --reps calls after one warm-up call, each synchronised (wall_times); the stage
times come from stage_times with sync_each=False.

    python tools/coverturn_time.py --variant 0 --ncont 121 --reps 5 --user
    python tools/coverturn_time.py --variant 1 --ncont 121 --reps 5
"""
import argparse

import numpy as np

import record_timing as rt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--variant', type=int, default=0)
    ap.add_argument('--ncont', type=int, default=121)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--ny', type=int, default=1801)
    ap.add_argument('--nx', type=int, default=3600)
    ap.add_argument('--select', default='main', choices=['all', 'circumpolar', 'main'])
    ap.add_argument('--user', action='store_true', help='also time trace_contours(join=\'device\', packed=True) + a numpy count')
    a = ap.parse_args()
    nat, ctx = rt.open_context()
    import xcontour_amd as xa
    ny, nx, N = a.ny, a.nx, a.ncont
    sel = nat.Context.OVERTURN_SELECT[a.select]
    q, qh, lat, lon, dlat, dlon = rt.synth_plane(ctx, nat, ny, nx, a.variant)
    lv = rt.levels_over(ctx, qh, N)
    dc = ctx.to_device(lv)

    def timed(fn):
        return rt.min_med_max(rt.wall_times(ctx, fn, a.reps), 1e6)

    def phases(call, profile, names):
        return rt.stage_times(ctx, call, profile, names, a.reps, sync_each=False)

    def median_us(v):
        return float(np.median([t * 1e3 for t in v]))

    seg = rt.SegmentRecords(ctx, nat, q, ny, nx, dc, N, True)
    seg.count()
    seg.size()
    total = seg.total
    print('variant %d ncont %d periodic, select %s: %d segments (%.1f MB of records, kept on the device); min / median / max of %d calls'
          % (a.variant, N, a.select, total, total * 48 / 1e6, a.reps))
    print('K12 count+emit    %s' % timed(seg.emit))

    # K16
    outs = [ctx.alloc(N * nx * b) for b in (4, 8, 8)] + [ctx.alloc(N * b) for b in (4, 8, 8, 4)]
    k16 = lambda: ctx._check(ctx.lib.xc_contour_overturning_dev(ctx.handle, *seg.recs, sel, *[b.ptr for b in outs]))
    print('K16 overturning   %s' % timed(k16))
    ph, pr = phases(k16, ctx.last_coverturn_profile, ('table_ms', 'rounds_ms', 'select_ms', 'count_ms'))
    for k, what in (('table_ms', 'clear, scatter, link, hand on clean'), ('rounds_ms', '%d doubling rounds over %d groups' % (pr['rounds'], pr['groups'])),
                    ('select_ms', 'roots, per-piece sums, pick'), ('count_ms', 'init, count, finish')):
        print('  %-8s        %s  (%s)' % (k[:-3], rt.min_med_max(ph[k], 1e3), what))
    print('  device sum      %10.1f us (medians)' % sum(median_us(v) for v in ph.values()))
    ncross = outs[0].download((N, nx), np.int32)
    mfe = outs[4].download((N,), np.int64)
    print('  %d levels have a main ring; %d (level, column) pairs are overturned (ncross >= 3), %d crossings in all'
          % (int((mfe >= 0).sum()), int((ncross >= 3).sum()), int(ncross.sum())))

    # K13 on the same records
    args = (ctx.handle,) + seg.recs + (dlat.ptr, dlon.ptr, 360.0, 0.0)
    dpc = ctx.alloc(N * 8)
    npiece = rt.count_then(ctx, lambda: ctx.lib.xc_contour_pieces_dev(*args, 0, dpc.ptr, *([None] * 8)), dpc, N)
    rec = [ctx.alloc(max(npiece, 1) * 8) for _ in range(8)]
    k13 = lambda: ctx._check(ctx.lib.xc_contour_pieces_dev(*args, npiece, dpc.ptr, *[b.ptr for b in rec]))
    print('K13 pieces        %s  (%d pieces)' % (timed(k13), npiece))
    ph, pr = phases(k13, ctx.last_cpiece_profile, ('table_ms', 'rounds_ms', 'roots_ms', 'reduce_ms'))
    for k in ph:
        print('  %-8s        %s' % (k[:-3], rt.min_med_max(ph[k], 1e3)))
    print('  device sum      %10.1f us (medians)' % sum(median_us(v) for v in ph.values()))
    for b in [seg.df, seg.dt, seg.dp, dc, seg.dn, dpc, q, dlat, dlon] + rec + outs:   # the host-array forms run with this memory released
        b.free()

    # the host-array forms
    print('Context.contour_overturning  %s' % timed(lambda: ctx.contour_overturning(qh[None], lv, periodic=True, select=a.select)))
    print('Context.contour_pieces       %s' % timed(lambda: ctx.contour_pieces(qh[None], lv, lat, lon, period=360.0)))
    if a.user:
        tr = xa.DataArray(qh, ('latitude', 'longitude'), {'latitude': lat, 'longitude': lon}, 'q')
        cm = xa.Contour2D(tr, np.ones(ny), {'X': 'longitude', 'Y': 'latitude'}, {'Y': 'latitude'}, dtype=np.float64)
        got = {}

        def trace():
            got['t'] = cm.trace_contours(lv, index=True, periodic=True, join='device', packed=True)

        def count():
            verts, voff, closed, winding, span = got['t']
            keep = np.ones(verts.shape[0], dtype=bool)
            keep[voff[1:][closed] - 1] = False                               # a ring repeats its first vertex
            c = verts[:, 1]
            on = keep & (c == np.floor(c)) & (verts[:, 0] != np.floor(verts[:, 0]))
            level = np.repeat(np.repeat(np.arange(N), np.diff(span, axis=1).ravel()), np.diff(voff))
            out = np.zeros((N, nx), dtype=np.int32)
            np.add.at(out, (level[on], c[on].astype(np.int64) % nx), 1)
            got['n'] = out
        print('trace_contours(join=\'device\', packed=True, index=True)  %s' % timed(trace))
        print('numpy count over its vertices (every piece)             %s  (%d crossings)' % (timed(count), int(got['n'].sum())))
    else:
        print('user route: not measured')


if __name__ == '__main__':
    main()
