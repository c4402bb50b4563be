#!/usr/bin/env python3
"""K12 timing: xc_contour_segments_dev on synthetic 3600 x 1801 float64 slabs (record_timing.synth_plane(ny, nx, variant, nslab=slabs):
variant 0 PV-like, 1 pure noise), N levels from the range of slab 0 (levels_over); the two passes of record_timing.SegmentRecords, each
under wall_mean.  Reports, per call,
  count   the count-only call (capacity 0): count pass + the two scan kernels + the one read-back of the total;
  full    the call into exactly sized buffers: the above + the emit pass (emit = full - count);
  join    xc_join_segments on the host, records already downloaded (skipped above --join-max segments);
  facade  Contour2D.find_contours(levels, index=True) on the same slab, host arrays in, polylines out (skipped likewise).
Wall-clock times around calls that end in a stream synchronisation.  --periodic: the periodic forms
(xc_contour_segments_periodic_dev, find_contours(periodic=True)): the ring of nx cell columns.

    python tools/cseg_time.py --variant 0 --ncont 121 --reps 5
    python tools/cseg_time.py --variant 0 --ncont 121 --reps 5 --periodic
"""
import argparse
import time

import numpy as np

import record_timing as rt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--slabs', type=int, default=1)
    ap.add_argument('--variant', type=int, default=0)
    ap.add_argument('--ncont', type=int, default=121)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--ny', type=int, default=1801)
    ap.add_argument('--nx', type=int, default=3600)
    ap.add_argument('--periodic', action='store_true', help='periodic X: the seam cell column is traced too')
    ap.add_argument('--join-max', type=int, default=30000000, help='most segments the host join and the facade call are timed on')
    a = ap.parse_args()
    nat, ctx = rt.open_context()
    import xcontour_amd as xa
    S, ny, nx, N = a.slabs, a.ny, a.nx, a.ncont
    q, qh, lat, lon, dlat, dlon = rt.synth_plane(ctx, nat, ny, nx, a.variant, nslab=S)
    lv = rt.levels_over(ctx, qh, N)
    seg = rt.SegmentRecords(ctx, nat, q, ny, nx, ctx.to_device(lv), N, a.periodic, nslab=S)
    t_count = rt.wall_mean(ctx, seg.count, a.reps)
    seg.size()
    cnt, total = seg.counts, seg.total
    cells = S * (ny - 1) * (nx if a.periodic else nx - 1)
    print('slabs %d variant %d ncont %d%s: %d segments (%.2f per cell, %.1f MB of records)'
          % (S, a.variant, N, ' periodic' if a.periodic else '', total, total / cells, total * 48 / 1e6))
    print('count pass  %10.1f us per call' % (t_count * 1e6))
    t_full = rt.wall_mean(ctx, seg.emit, a.reps)
    print('count+emit  %10.1f us per call  (emit pass %.1f us, %.0f GB/s of records)'
          % (t_full * 1e6, (t_full - t_count) * 1e6, total * 48 / max(t_full - t_count, 1e-9) / 1e9))
    if total <= a.join_max:
        ef, et = seg.df.download((total,), np.int64), seg.dt.download((total,), np.int64)
        off = np.concatenate([[0], np.cumsum(cnt.ravel().astype(np.int64))])
        t0 = time.perf_counter()
        _, poff, closed, _ = nat.join_segments(off, ef, et)
        print('host join   %10.1f us  (%d polylines, %d of them rings)' % ((time.perf_counter() - t0) * 1e6, closed.size, int(closed.sum())))
        tr = xa.DataArray(qh, ('latitude', 'longitude'), {'latitude': lat, 'longitude': lon}, 'q')
        cm = xa.Contour2D(tr, np.ones(ny), {'X': 'longitude', 'Y': 'latitude'}, {'Y': 'latitude'}, dtype=np.float64)
        cm.find_contours(lv[:2], index=True, periodic=a.periodic)
        t0 = time.perf_counter()
        out = cm.find_contours(lv, index=True, periodic=a.periodic)
        print('facade      %10.1f us  (find_contours of slab 0, %d polylines kept)' % ((time.perf_counter() - t0) * 1e6, sum(len(p) for p in out)))
    else:
        print('host join   not measured (more than --join-max segments)')
        print('facade      not measured (more than --join-max segments)')


if __name__ == '__main__':
    main()
