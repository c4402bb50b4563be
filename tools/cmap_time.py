#!/usr/bin/env python3
"""K25 timing: xc_contour_map_dev on synthetic 1801 x 3600 float64 slabs made on the device (record_timing.synth_plane: variant 0
PV-like -- neighbouring lanes share a bracket --, 1 pure noise -- they never do), N levels from the range of slab 0 (levels_over),
nv value vectors, against K4 xc_grad2_dev on the same slabs in the same process: K4 also moves 16 bytes per cell and DESIGN.md
records it at the copy ceiling.  Times are HIP events around `reps` calls after a warm one, the two kernels alternating; per line
the time per call, the bytes moved per cell and the rate, and the ratio to K4.

    python tools/cmap_time.py                       # one slab and 64 slabs, nv 1 and 2, both variants
    python tools/cmap_time.py --slabs 64 --nv 8 --ncont 201 --variant 1
"""
import argparse

import numpy as np

import record_timing as rt


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


def measure(ctx, nat, S, ny, nx, N, nv, variant, reps, rounds):
    import ctypes as C
    q, qh, lat, lon, dlat, dlon = rt.synth_plane(ctx, nat, ny, nx, variant, nslab=S)
    lv = rt.levels_over(ctx, qh, N)
    dc = ctx.to_device(lv)
    vecs = [ctx.to_device(np.sin(np.linspace(0.0, 3.0, N) * (v + 1))) for v in range(nv)]
    outs = [ctx.alloc(S * ny * nx * 8) for _ in range(max(nv, 1))]
    ones = ctx.to_device(np.ones(ny))
    fp, op, fl = (C.c_void_p * nv)(*[b.ptr for b in vecs]), (C.c_void_p * nv)(*[b.ptr for b in outs[:nv]]), (C.c_int * nv)(*[0] * nv)

    def k25():
        ctx._check(ctx.lib.xc_contour_map_dev(ctx.handle, q.ptr, nat.XC_F64, S, ny, nx, dc.ptr, N, 0, nv, fp, fl, op, nat.XC_F64))

    def k4():
        ctx._check(ctx.lib.xc_grad2_dev(ctx.handle, q.ptr, nat.XC_F64, S, ny, nx, ones.ptr, ones.ptr, 1, outs[0].ptr))
    # the two kernels alternate, `rounds` times: the spread shows with the means
    t25, t4 = [], []
    for _ in range(rounds):
        t4.append(event_ms(ctx, k4, reps))
        t25.append(event_ms(ctx, k25, reps))
    cells = S * ny * nx
    gbs = lambda ms, b: cells * b / (ms * 1e-3) / 1e9
    m25, m4 = float(np.median(t25)), float(np.median(t4))
    print('slabs %3d variant %d N %d nv %d | K25 %9.1f us (%s) %2d B/cell %6.0f GB/s | K4 %9.1f us (%s) 16 B/cell %6.0f GB/s | K25 / K4 %.2f'
          % (S, variant, N, nv, m25 * 1e3, rt.min_med_max(t25, 1e3).strip(), 8 + 8 * nv, gbs(m25, 8 + 8 * nv), m4 * 1e3,
             rt.min_med_max(t4, 1e3).strip(), gbs(m4, 16), m25 / m4))
    for b in [q, dlat, dlon, dc, ones] + vecs + outs:                # (the next configuration runs with this memory released)
        b.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--slabs', type=int, default=0, help='0: one slab, then 64')
    ap.add_argument('--variant', type=int, default=-1, help='-1: both')
    ap.add_argument('--nv', type=int, default=0, help='0: 1, then 2')
    ap.add_argument('--ncont', type=int, default=201)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--ny', type=int, default=1801)
    ap.add_argument('--nx', type=int, default=3600)
    a = ap.parse_args()
    nat, ctx = rt.open_context()
    for S in ([a.slabs] if a.slabs else [1, 64]):
        for variant in ([a.variant] if a.variant >= 0 else [0, 1]):
            for nv in ([a.nv] if a.nv else [1, 2]):
                measure(ctx, nat, S, a.ny, a.nx, a.ncont, nv, variant, max(2, a.reps // (4 if S > 8 else 1)), a.rounds)


if __name__ == '__main__':
    main()
