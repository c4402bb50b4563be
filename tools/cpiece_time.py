#!/usr/bin/env python3
"""K13 timing: xc_contour_pieces_dev on one synthetic 1801 x 3600 float64 slab (record_timing.synth_plane(ny, nx, variant): variant 0
PV-like, 1 pure noise), N levels over the field's range (levels_over) and K12's records of them (SegmentRecords, periodic or not).  Reports, per call,
  K12      xc_contour_segments_dev into exactly sized device buffers (count + emit), wall clock around the synchronising call;
  K13      xc_contour_pieces_dev on those buffers, wall clock, and inside it from HIP events (xc_set_kernel_timing):
           table     clearing the edge tables, scatter, link, and handing the tables on clean
           rounds    the pointer-doubling rounds (with their number, summed over the groups of ranges)
           roots     roots, slots and their broadcast
           reduce    the per-piece reductions (init, one pass over the segments, finish)
  download the piece table brought to the host (six 8-byte and two 4-byte columns).
With --host (variant 0 is what it is meant for): the parent commit's route to the same numbers -- Context.contour_segments (records
to the host), join_segments, and numpy reductions over the walk (np.add.reduceat of the segment lengths, shoelace terms and row
extents per polyline).  --periodic: the periodic forms.

    python tools/cpiece_time.py --variant 0 --ncont 121 --reps 3 --host
    python tools/cpiece_time.py --variant 1 --ncont 121 --reps 3
"""
import argparse
import time

import numpy as np

import record_timing as rt


def host_route(ctx, nat, qh, lv, lat, lon, periodic):
    """segments to the host, the host join, numpy reductions per polyline -> the three times (s) and the number of polylines"""
    ny, nx = qh.shape
    t0 = time.perf_counter()
    cnt, ef, et, pts = ctx.contour_segments(qh[None], lv, periodic=periodic)
    t1 = time.perf_counter()
    off = np.concatenate([[0], np.cumsum(cnt.ravel().astype(np.int64))])
    walk, poff, closed, _ = nat.join_segments(off, ef, et)
    t2 = time.perf_counter()
    xe = np.concatenate([lon, [lon[0] + 360.0]]) if periodic else lon
    p = pts[walk]
    y1, y2 = np.interp(p[:, 0], np.arange(ny), lat), np.interp(p[:, 2], np.arange(ny), lat)
    x1, x2 = np.interp(p[:, 1], np.arange(xe.size), xe), np.interp(p[:, 3], np.arange(xe.size), xe)
    heads = poff[:-1]
    length = np.add.reduceat(np.hypot(x1 - x2, y1 - y2), heads)
    area = np.add.reduceat(0.5 * (y1 + y2) * (x1 - x2), heads)
    rmin = np.minimum.reduceat(np.minimum(p[:, 0], p[:, 2]), heads)
    rmax = np.maximum.reduceat(np.maximum(p[:, 0], p[:, 2]), heads)
    nseg = np.diff(poff)
    t3 = time.perf_counter()
    assert length.size == area.size == rmin.size == rmax.size == nseg.size == closed.size
    return t1 - t0, t2 - t1, t3 - t2, closed.size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--variant', type=int, default=0)
    ap.add_argument('--ncont', type=int, default=121)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--ny', type=int, default=1801)
    ap.add_argument('--nx', type=int, default=3600)
    ap.add_argument('--periodic', action='store_true', help='periodic X: the seam cell column is traced too')
    ap.add_argument('--host', action='store_true', help='also time the route through the host join')
    a = ap.parse_args()
    nat, ctx = rt.open_context()
    ny, nx, N = a.ny, a.nx, a.ncont
    q, qh, lat, lon, dlat, dlon = rt.synth_plane(ctx, nat, ny, nx, a.variant)
    lv = rt.levels_over(ctx, qh, N)
    seg = rt.SegmentRecords(ctx, nat, q, ny, nx, ctx.to_device(lv), N, a.periodic)
    seg.count()
    seg.size()
    total = seg.total
    print('variant %d ncont %d%s: %d segments (%.1f MB of records, kept on the device)'
          % (a.variant, N, ' periodic' if a.periodic else '', total, total * 48 / 1e6))
    t12 = rt.wall_mean(ctx, seg.emit, a.reps)
    print('K12 count+emit   %10.1f us per call' % (t12 * 1e6))
    # K13: a count-only call sizes the record arrays
    args = (ctx.handle,) + seg.recs + (dlat.ptr, dlon.ptr, 360.0, 0.0)
    dpc = ctx.alloc(N * 8)
    npiece = rt.count_then(ctx, lambda: ctx.lib.xc_contour_pieces_dev(*args, 0, dpc.ptr, *([None] * 8)), dpc, N)
    rec = [ctx.alloc(max(npiece, 1) * 8) for _ in range(8)]
    call = lambda: ctx._check(ctx.lib.xc_contour_pieces_dev(*args, npiece, dpc.ptr, *[b.ptr for b in rec]))
    t13 = rt.wall_mean(ctx, call, a.reps)
    acc, pr = rt.stage_times(ctx, call, ctx.last_cpiece_profile, ('table_ms', 'rounds_ms', 'roots_ms', 'reduce_ms'), a.reps, sync_each=False)
    acc = {k: rt.mean_of(v) for k, v in acc.items()}
    closed = rec[2].download((npiece,), np.int32)
    print('K13 pieces       %10.1f us per call  (%d pieces, %d of them rings; %d groups of ranges)'
          % (t13 * 1e6, npiece, int(closed.sum()), pr['groups']))
    print('  table          %10.1f us  (clear, scatter, link, hand on clean)' % (acc['table_ms'] * 1e3))
    print('  rounds         %10.1f us  (%d doubling rounds over all groups)' % (acc['rounds_ms'] * 1e3, pr['rounds']))
    print('  roots          %10.1f us  (roots, slots, broadcast)' % (acc['roots_ms'] * 1e3))
    print('  reduce         %10.1f us  (init, reductions, finish)' % (acc['reduce_ms'] * 1e3))
    t0 = time.perf_counter()
    for _ in range(a.reps):
        cols = [rec[k].download((npiece,), np.int64 if k < 2 else np.float64) for k in (0, 1, 4, 5, 6, 7)]
        cols += [rec[k].download((npiece,), np.int32) for k in (2, 3)]
    print('download         %10.1f us  (%.1f MB of piece records)' % ((time.perf_counter() - t0) / a.reps * 1e6, npiece * 56 / 1e6))
    if a.host:
        host_route(ctx, nat, qh[:64], lv, lat[:64], lon, a.periodic)                      # (warm-up on a strip)
        ts, tj, tr, npoly = host_route(ctx, nat, qh, lv, lat, lon, a.periodic)
        print('host route: contour_segments %.3f s, join_segments %.3f s, numpy reductions over the walk %.3f s (%d polylines)'
              % (ts, tj, tr, npoly))
        assert npoly == npiece
    else:
        print('host route: not measured')


if __name__ == '__main__':
    main()
