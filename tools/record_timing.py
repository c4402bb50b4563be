"""What the timing tools (tools/c*_time.py, tools/local_clen_time.py) and the trace tools (tools/*_trace.py) share: the synthetic plane,
K12's two-pass record set-up, the count-only idiom, the wall and stage timers and the two line shapes they print.  A tool imports it
as a plain module beside it (`import record_timing`: the script's own directory is sys.path[0]).  What a tool does differently from the
others it states as an argument here (`offset`, `sync_each`, `warm`, `sync`, `with_sum`).

Device buffers: no tool frees its buffers at the end.  A tool is a one-shot process; the buffers belong to its context, which frees
them when it is closed or collected, and the process's exit returns the device memory in any case -- nothing is measured after the last
line.  A tool frees buffers only in the MIDDLE, where measured lines follow that ran with that memory released before
(coverturn_time.py before the host-array forms, cjoin_time.py after the download of the plane, cline_time.py the levels of a variant
before the next one, the two trace tools the buffers of the periodic pass before the plain one)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def open_context(root=ROOT):
    """the checkout `root` first on sys.path -> (xcontour_amd._native of it, its process-wide context of device 0)"""
    sys.path.insert(0, os.path.abspath(root))
    from xcontour_amd import _native as nat
    return nat, nat.default_context(0)


def lat_lon(ctx, ny, nx):
    """-> lat (-90 ... 90, ny nodes), lon (0 ... 360 without the end, nx nodes) in degrees, and their device copies"""
    lat = np.linspace(-90.0, 90.0, ny)
    lon = np.linspace(0.0, 360.0, nx, endpoint=False)
    return lat, lon, ctx.to_device(lat), ctx.to_device(lon)


def synth_fill(ctx, nat, q, nslab, ny, nx, dlat, dlon, variant, seed=1):
    """xc_synth_dev into the float64 slabs of `q` (variant 0: PV-like, 1: pure noise)"""
    ctx._check(ctx.lib.xc_synth_dev(ctx.handle, q.ptr, nat.XC_F64, nslab, ny, nx, dlat.ptr, dlon.ptr, seed, variant))


def synth_plane(ctx, nat, ny, nx, variant, nslab=1, seed=1, host=True):
    """`nslab` synthetic float64 slabs made on the device -> (q, qh, lat, lon, dlat, dlon): the device slabs, the host copy of slab 0
    (ny, nx) -- None with host=False: no download --, lat_lon()"""
    lat, lon, dlat, dlon = lat_lon(ctx, ny, nx)
    q = ctx.alloc(nslab * ny * nx * 8)
    synth_fill(ctx, nat, q, nslab, ny, nx, dlat, dlon, variant, seed)
    return q, (q.download((ny, nx), np.float64) if host else None), lat, lon, dlat, dlon


def levels_over(ctx, qh, N):
    """N levels from the minimum to the maximum of the plane `qh` (Context.minmax)"""
    mm = ctx.minmax(qh.reshape(1, -1))[0]
    return np.linspace(mm[0], mm[1], N)


def cos_weights(lat, ny, nx, offset=0.0):
    """the weight plane cos(latitude) [+ offset] per node, (ny, nx) float64"""
    c = np.cos(np.deg2rad(lat))[:, None]
    return np.ascontiguousarray(np.broadcast_to(c + offset if offset else c, (ny, nx)))


def count_only(ctx, count_only_call):
    """make a count-only call: status 0, or 1 -- the counts exceed the capacity, which is what the call is for --; anything else raises"""
    rc = count_only_call()
    if rc not in (0, 1):
        ctx._check(rc)


def counts_then(ctx, count_only_call, count_buf, n):
    """count_only(), then the `n` uint64 counts it left in `count_buf`"""
    count_only(ctx, count_only_call)
    return count_buf.download((n,), np.uint64)


def count_then(ctx, count_only_call, count_buf, n):
    """counts_then(), summed"""
    return int(counts_then(ctx, count_only_call, count_buf, n).sum())


class SegmentRecords(object):
    """K12's segment records of `N` levels `dc` on the slabs `q`, kept on the device, in the library's two passes: count() -- the
    count-only call into `dn` --, size() -- the counts to the host (`counts`, `total`) and the exactly sized `df`, `dt`, `dp` --, emit()
    -- the sized call.  A tool that times K12 itself times count or emit; the others take segment_records().  `recs`: what the argument
    lists of the record-consuming entry points start with behind the handle."""

    def __init__(self, ctx, nat, q, ny, nx, dc, N, periodic, nslab=1):
        self.ctx, self.shape = ctx, (nslab, N)
        self.f = ctx.lib.xc_contour_segments_periodic_dev if periodic else ctx.lib.xc_contour_segments_dev
        self.head = (ctx.handle, q.ptr, nat.XC_F64, nslab, ny, nx, dc.ptr, N, 0)
        self.plane = (ny, nx, 1 if periodic else 0)
        self.dn = ctx.alloc(nslab * N * 8)

    def count(self):
        count_only(self.ctx, lambda: self.f(*self.head, 0, self.dn.ptr, None, None, None))

    def size(self):
        self.counts = self.dn.download(self.shape, np.uint64)
        self.total = int(self.counts.sum())
        self.df, self.dt, self.dp = (self.ctx.alloc(max(self.total, 1) * b) for b in (8, 8, 32))
        self.recs = (self.shape[1], self.dn.ptr, self.df.ptr, self.dt.ptr, self.dp.ptr) + self.plane

    def emit(self):
        self.ctx._check(self.f(*self.head, self.total, self.dn.ptr, self.df.ptr, self.dt.ptr, self.dp.ptr))


def segment_records(ctx, nat, q, ny, nx, dc, N, periodic, nslab=1):
    """the two-pass K12 set-up, each pass once -> SegmentRecords with dn, df, dt, dp, counts, total, recs"""
    seg = SegmentRecords(ctx, nat, q, ny, nx, dc, N, periodic, nslab)
    seg.count()
    seg.size()
    seg.emit()
    return seg


def wall_times(ctx, call, reps, sync=True):
    """one warm call, then `reps` calls, each synchronised (sync=False: a call that ends in a download of its own) -> their times (s)"""
    call()
    if sync:
        ctx.sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        if sync:
            ctx.sync()
        ts.append(time.perf_counter() - t0)
    return ts


def wall_mean(ctx, call, reps):
    """one warm call, then `reps` calls and ONE synchronisation behind them -> the mean time of a call (s)"""
    call()
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    ctx.sync()
    return (time.perf_counter() - t0) / reps


def stage_times(ctx, call, profile, keys, reps, sync_each, warm=True):
    """under set_kernel_timing(True): one warm call (warm=False: none), then `reps` calls, `profile()` read after each; sync_each: the
    stream is synchronised after every call, the warm one too -> ({key: the `reps` values of profile()[key], in ms}, the last profile).
    Kernel timing is off again afterwards, also when a call raises."""
    acc, pr = {k: [] for k in keys}, None
    ctx.set_kernel_timing(True)
    try:
        for rep in range(reps + 1 if warm else reps):
            call()
            if sync_each:
                ctx.sync()
            if warm and rep == 0:
                continue
            pr = profile()
            for k in keys:
                acc[k].append(pr[k])
    finally:
        ctx.set_kernel_timing(False)
    return acc, pr


def mean_of(values):
    """the mean the tools print: the sum of value / n in order"""
    return sum(v / len(values) for v in values)


def min_med_max(values, scale):
    """-> 'min / median / max us' of `values` times `scale`"""
    v = [t * scale for t in values]
    return '%10.1f / %10.1f / %10.1f us' % (min(v), float(np.median(v)), max(v))


def mean_line(name, wall, acc, pr, with_sum=True):
    """-> 'name wall ms | stage means | [sum |] rounds, groups': `wall` in s, `acc` the stage means in ms, `pr` the last profile"""
    return ('%-22s wall %9.3f ms | %s | %s%d rounds, %d groups'
            % (name, wall * 1e3, ', '.join('%s %8.3f' % kv for kv in acc.items()), 'sum %8.3f | ' % sum(acc.values()) if with_sum else '',
               pr['rounds'], pr['groups']))


def report_means(ctx, name, call, profile, keys, reps, with_sum=True):
    """wall_mean(), then stage_times() without a synchronisation per call; prints the mean_line() -> (wall in s, {key: mean in ms})"""
    wall = wall_mean(ctx, call, reps)
    acc, pr = stage_times(ctx, call, profile, keys, reps, sync_each=False)
    acc = {k: mean_of(v) for k, v in acc.items()}
    print(mean_line(name, wall, acc, pr, with_sum))
    return wall, acc
