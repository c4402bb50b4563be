#!/usr/bin/env python3
"""K26 timing: contour lengths at the ruler ratios 1, 2, 4, 8, 16, 32 of one synthetic 1801 x 3600 float64 slab made on the device
(record_timing.synth_plane: variant 0 PV-like, 1 pure noise), `ncont` levels from the range of the slab, great-circle lengths.

  one call      Context.contour_lengths_scales on the host array: one upload, six coarsen + K10 rounds, one download (wall clock
                around the synchronising call), and xc_contour_lengths_scales_dev on the device slab (HIP events);
  six calls     what the same workflow costs without K26: the slab block-averaged on the host with numpy (timed apart: it is not
                GPU work) and Context.contour_lengths called on each of the six planes -- six uploads, six K10 launches;
  the kernel    xc_coarsen_dev alone per ratio, HIP events around `reps` calls after a warm one: time, and the bytes of the fine
                plane over that time (every ratio reads all of it but the trimmed tail and writes 1 / r^2 of it).

    python tools/cscale_time.py
    python tools/cscale_time.py --variant 1 --ncont 41 --reps 5
"""
import argparse
import time

import numpy as np

import record_timing as rt

RATIOS = [1, 2, 4, 8, 16, 32]


def event_ms(ctx, call, reps):
    """one warm call, then `reps` calls between two events -> ms per call"""
    call()
    ctx.sync()
    e0, e1 = ctx.event(), ctx.event()
    ctx.record(e0)
    for _ in range(reps):
        call()
    ctx.record(e1)
    ctx.sync()
    return ctx.elapsed_ms(e0, e1) / reps


def host_block_mean(q, r):
    """the plane a user would make on the host (numpy's own summation order: a stand-in for timing, not K26's rule)"""
    cy, cx = q.shape[0] // r, q.shape[1] // r
    return q if r == 1 else np.ascontiguousarray(q[:cy * r, :cx * r].reshape(cy, r, cx, r).mean(axis=(1, 3)))


def measure(ctx, nat, ny, nx, N, variant, reps, rounds):
    import ctypes as C
    q, qh, lat, lon, dlat, dlon = rt.synth_plane(ctx, nat, ny, nx, variant)
    lev = rt.levels_over(ctx, qh, N + 2)[1:-1]
    y, x = np.deg2rad(lat), np.deg2rad(lon)
    R = 6371200.0
    q3 = qh[None]
    name = 'PV-like' if variant == 0 else 'noise'

    one = rt.wall_times(ctx, lambda: ctx.contour_lengths_scales(q3, lev, y, x, RATIOS, radius=R), reps, sync=False)
    t0 = time.perf_counter()
    planes = [host_block_mean(qh, r) for r in RATIOS]
    t_host = time.perf_counter() - t0
    mean1 = lambda c, r: np.ascontiguousarray(c[:c.size // r * r].reshape(-1, r).mean(axis=1))
    coords = [(mean1(y, r), mean1(x, r)) for r in RATIOS]

    def six():
        for p, (cy, cx) in zip(planes, coords):
            ctx.contour_lengths(p[None], lev, cy, cx, radius=R)
    six_t = rt.wall_times(ctx, six, reps, sync=False)
    print('%-8s N %d | one call %s | six calls %s | host block means of the six planes %.1f ms (numpy, not in either)'
          % (name, N, rt.min_med_max(one, 1e6).strip(), rt.min_med_max(six_t, 1e6).strip(), t_host * 1e3))

    dy, dx, dc = ctx.to_device(y), ctx.to_device(x), ctx.to_device(lev)
    dl = ctx.alloc(len(RATIOS) * N * 8)
    rr = (C.c_int * len(RATIOS))(*RATIOS)

    def dev():
        ctx._check(ctx.lib.xc_contour_lengths_scales_dev(ctx.handle, q.ptr, nat.XC_F64, 1, ny, nx, dy.ptr, dx.ptr, 0.0, R, rr, len(RATIOS), 0,
                                                         dc.ptr, N, 0, dl.ptr, None))

    def k10():
        ctx._check(ctx.lib.xc_contour_lengths_dev(ctx.handle, q.ptr, nat.XC_F64, 1, ny, nx, dy.ptr, dx.ptr, R, dc.ptr, N, 0, dl.ptr, None))
    td = [event_ms(ctx, dev, reps) for _ in range(rounds)]
    tk = [event_ms(ctx, k10, reps) for _ in range(rounds)]
    print('%-8s N %d | xc_contour_lengths_scales_dev, six ratios %s | xc_contour_lengths_dev on the fine plane alone %s'
          % (name, N, rt.min_med_max(td, 1e3).strip(), rt.min_med_max(tk, 1e3).strip()))

    out = ctx.alloc((ny // 2) * (nx // 2) * 8)
    for r in RATIOS[1:]:
        def kern():
            ctx._check(ctx.lib.xc_coarsen_dev(ctx.handle, q.ptr, nat.XC_F64, 1, ny, nx, r, 0, out.ptr))
        ts = [event_ms(ctx, kern, reps * 4) for _ in range(rounds)]
        read = (ny // r * r) * (nx // r * r) * 8
        print('%-8s k_coarsen ratio %2d | %s | %.1f MB read | %6.0f GB/s (median)'
              % (name, r, rt.min_med_max(ts, 1e3).strip(), read / 1e6, read / (float(np.median(ts)) * 1e-3) / 1e9))
    for b in (q, dlat, dlon, dy, dx, dc, dl, out):
        b.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--variant', type=int, default=-1, help='-1: both')
    ap.add_argument('--ncont', type=int, default=121)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--ny', type=int, default=1801)
    ap.add_argument('--nx', type=int, default=3600)
    a = ap.parse_args()
    nat, ctx = rt.open_context()
    for variant in ([a.variant] if a.variant >= 0 else [0, 1]):
        measure(ctx, nat, a.ny, a.nx, a.ncont, variant, a.reps, a.rounds)


if __name__ == '__main__':
    main()
