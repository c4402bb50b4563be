# -*- coding: utf-8 -*-
"""tools/record_timing.py -- what the timing and trace tools under tools/ share -- pinned without a GPU on the stand-in library of
standin_lib.py: the synthetic plane's one library call and its allocations, K12's two passes (the count-only call with capacity 0 and
null record pointers, the sized call with the downloaded total, the record buffers of max(total, 1) * (8, 8, 32) bytes), the count-only
idiom (status 1 is success, a negative status raises), how often the timers call and synchronise, that kernel timing is off after
stage_times() whatever the call did, and the text of the two line shapes."""
import os
import sys

import numpy as np
import pytest

from standin_lib import _Lib

from xcontour_amd import _native as nat

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import record_timing as rt  # noqa: E402

NY, NX, N = 6, 8, 4
_EXTRA = ('xc_synth_dev', 'xc_set_kernel_timing', 'xc_sync')


class _ToolLib(_Lib):
    """the stand-in, which also records (name, arguments) of the three entry points in _EXTRA in `extra`, and the bytes of every
    download in `d2h`"""

    def __init__(self):
        _Lib.__init__(self)
        self.extra, self.d2h = [], []

    def __getattr__(self, name):
        if name in _EXTRA:
            return lambda *a: (self.extra.append((name, tuple(a[1:]))), 0)[1]
        if name == 'xc_memcpy_d2h':
            return lambda h, dst, src, n: (self.d2h.append(int(n)), self._d2h(h, dst, src, n))[1]
        return _Lib.__getattr__(self, name)

    def named(self, name):
        return [a for n, a in self.extra if n == name]


@pytest.fixture
def ctx():
    c = nat.Context.__new__(nat.Context)
    c.lib, c.handle, c.device = _ToolLib(), None, 0
    c._buffers, c._resident, c._staged, c._ev_pool = [], {}, [], []
    c.max_batch_bytes = 8 << 30
    return c


def D(nbytes, off=0):
    return ('dev', nbytes, off)


@pytest.mark.parametrize('nslab, host', [(1, True), (3, True), (2, False)])
def test_synth_plane(ctx, nslab, host):
    lib = ctx.lib
    q, qh, lat, lon, dlat, dlon = rt.synth_plane(ctx, nat, NY, NX, 1, nslab=nslab, seed=7, host=host)
    assert lib.mallocs == [NY * 8, NX * 8, nslab * NY * NX * 8]                   # lat, lon, the slabs: in this order
    (a,) = lib.named('xc_synth_dev')
    assert tuple(lib.where(v) for v in a) == (D(nslab * NY * NX * 8), nat.XC_F64, nslab, NY, NX, D(NY * 8), D(NX * 8), 7, 1)
    assert np.array_equal(lat, np.linspace(-90.0, 90.0, NY)) and np.array_equal(lon, np.arange(NX) * (360.0 / NX))
    assert (dlat.nbytes, dlon.nbytes, q.nbytes) == (NY * 8, NX * 8, nslab * NY * NX * 8)
    if host:
        assert qh.shape == (NY, NX) and qh.dtype == np.float64 and lib.d2h == [NY * NX * 8]      # slab 0 alone comes to the host
    else:
        assert qh is None and lib.d2h == []
    assert lib.calls == []                                                       # nothing else was computed


def test_levels_and_weights(ctx):
    lv = rt.levels_over(ctx, np.zeros((NY, NX)), N)
    assert ctx.lib.calls == [('xc_minmax', 1)] and lv.shape == (N,)
    lat = np.linspace(-90.0, 90.0, NY)
    w = rt.cos_weights(lat, NY, NX)
    assert w.shape == (NY, NX) and w.flags['C_CONTIGUOUS'] and np.array_equal(w[:, 3], np.cos(np.deg2rad(lat)))
    assert np.array_equal(rt.cos_weights(lat, NY, NX, offset=1e-3), w + 1e-3)


@pytest.mark.parametrize('periodic, name', [(False, 'xc_contour_segments_dev'), (True, 'xc_contour_segments_periodic_dev')])
@pytest.mark.parametrize('nslab', [1, 3])
@pytest.mark.parametrize('found', [2, 0])
def test_segment_records(ctx, periodic, name, nslab, found):
    lib = ctx.lib
    q, dc = ctx.alloc(nslab * NY * NX * 8), ctx.alloc(N * 8)
    lib.mallocs = []
    if found:
        lib.d2h_u64 = lambda l: found                  # every count reads `found`: the count-only call answers 1, as the library's does
    seg = rt.segment_records(ctx, nat, q, NY, NX, dc, N, periodic, nslab=nslab)
    total = found * nslab * N
    assert seg.total == total and seg.counts.shape == (nslab, N) and int(seg.counts.sum()) == total
    assert lib.calls == [(name, nslab)] * 2
    head = (None, D(q.nbytes), nat.XC_F64, nslab, NY, NX, D(N * 8), N, 0)
    cap = max(total, 1)
    count, sized = [tuple(lib.where(v) for v in a) for _, a in lib.args]
    assert count == head + (0, D(nslab * N * 8), None, None, None)               # capacity 0, null record pointers
    assert sized == head + (total, D(nslab * N * 8), D(cap * 8), D(cap * 8), D(cap * 32))        # the downloaded total
    assert len(set(lib.args[1][1][10:14])) == 4                                   # four buffers
    assert lib.mallocs == [nslab * N * 8, cap * 8, cap * 8, cap * 32]
    assert lib.d2h == [nslab * N * 8]                                            # the counts come to the host once
    assert seg.recs == (N, seg.dn.ptr, seg.df.ptr, seg.dt.ptr, seg.dp.ptr, NY, NX, 1 if periodic else 0)
    assert (seg.dn.ptr, seg.df.ptr, seg.dt.ptr, seg.dp.ptr) == lib.args[1][1][10:14]


def test_segment_records_passes_apart(ctx):
    """a tool that times K12 itself makes the passes one by one: every count() and every emit() is one library call"""
    lib = ctx.lib
    lib.d2h_u64 = lambda l: 2
    seg = rt.SegmentRecords(ctx, nat, ctx.alloc(NY * NX * 8), NY, NX, ctx.alloc(N * 8), N, False)
    for _ in range(3):
        seg.count()
    assert [a[9] for _, a in lib.args] == [0, 0, 0] and lib.d2h == []
    seg.size()
    assert seg.total == 2 * N and lib.d2h == [N * 8] and len(lib.args) == 3
    seg.emit()
    seg.emit()
    assert [a[9] for _, a in lib.args] == [0, 0, 0, 2 * N, 2 * N]


@pytest.mark.parametrize('status', [0, 1])
def test_count_then_takes_0_and_1_as_success(ctx, status):
    ctx.lib.d2h_u64 = lambda l: 2
    made = []
    buf = ctx.alloc(N * 8)
    assert rt.count_then(ctx, lambda: (made.append(1), status)[1], buf, N) == 2 * N
    assert made == [1] and ctx.lib.d2h == [N * 8]
    assert rt.counts_then(ctx, lambda: status, buf, N).tolist() == [2] * N


@pytest.mark.parametrize('status', [-1, -7, 2])
def test_count_then_raises_on_any_other_status(ctx, status):
    buf = ctx.alloc(N * 8)
    with pytest.raises(nat.XContourHipError) as e:
        rt.count_then(ctx, lambda: status, buf, N)
    assert e.value.code == status and ctx.lib.d2h == []                          # nothing is downloaded behind a failed call


def _profile():
    """profile() of a fake entry: 'a_ms' counts the reads"""
    n = []
    return lambda: (n.append(1), {'a_ms': float(len(n)), 'b_ms': 10.0 * len(n), 'rounds': len(n), 'groups': 1})[1]


@pytest.mark.parametrize('reps', [1, 3])
@pytest.mark.parametrize('sync_each', [False, True])
def test_stage_times(ctx, reps, sync_each):
    lib, made = ctx.lib, []
    acc, pr = rt.stage_times(ctx, lambda: made.append(1), _profile(), ('a_ms', 'b_ms'), reps, sync_each)
    assert len(made) == 1 + reps                                                 # one warm call, then the repeats
    assert acc == {'a_ms': [float(k) for k in range(1, reps + 1)], 'b_ms': [10.0 * k for k in range(1, reps + 1)]}
    assert pr['rounds'] == reps                                                  # the profile is not read behind the warm call
    assert lib.named('xc_set_kernel_timing') == [(1,), (0,)]
    assert len(lib.named('xc_sync')) == (1 + reps if sync_each else 0)
    assert lib.extra[0][0] == lib.extra[-1][0] == 'xc_set_kernel_timing'         # every sync lies between the two switches


def test_stage_times_without_a_warm_call(ctx):
    made = []
    acc, pr = rt.stage_times(ctx, lambda: made.append(1), _profile(), ('a_ms',), 2, False, warm=False)
    assert len(made) == 2 and acc == {'a_ms': [1.0, 2.0]} and ctx.lib.named('xc_set_kernel_timing') == [(1,), (0,)]


@pytest.mark.parametrize('fail_at', [0, 2])
def test_stage_times_switches_timing_off_when_the_call_raises(ctx, fail_at):
    made = []

    def call():
        made.append(1)
        if len(made) - 1 == fail_at:
            raise nat.XContourHipError(-5, 'scripted')
    with pytest.raises(nat.XContourHipError):
        rt.stage_times(ctx, call, _profile(), ('a_ms',), 3, True)
    assert len(made) == fail_at + 1 and ctx.lib.named('xc_set_kernel_timing') == [(1,), (0,)]


def test_wall_timers(ctx):
    lib, made = ctx.lib, []
    ts = rt.wall_times(ctx, lambda: made.append(1), 3)
    assert len(ts) == 3 and min(ts) >= 0.0 and len(made) == 4 and len(lib.named('xc_sync')) == 4     # each call synchronised
    rt.wall_times(ctx, lambda: made.append(1), 2, sync=False)
    assert len(made) == 7 and len(lib.named('xc_sync')) == 4
    assert rt.wall_mean(ctx, lambda: made.append(1), 3) >= 0.0
    assert len(made) == 11 and len(lib.named('xc_sync')) == 6                    # one behind the warm call, one behind the repeats
    assert lib.named('xc_set_kernel_timing') == []


def test_report_means_and_the_two_line_shapes(ctx, capsys):
    made = []
    wall, acc = rt.report_means(ctx, 'K19 piece tree', lambda: made.append(1), _profile(), ('a_ms', 'b_ms'), 2)
    assert len(made) == 2 * (1 + 2) and acc == {'a_ms': 1.5, 'b_ms': 15.0}
    assert len(ctx.lib.named('xc_sync')) == 2 and ctx.lib.named('xc_set_kernel_timing') == [(1,), (0,)]
    assert capsys.readouterr().out == rt.mean_line('K19 piece tree', wall, acc, {'rounds': 2, 'groups': 1}) + '\n'
    pr = {'rounds': 22, 'groups': 6}
    acc = {'table_ms': 1.25, 'walk_ms': 40.0}
    assert rt.mean_line('K18 piece interiors', 0.0655, acc, pr) == \
        'K18 piece interiors    wall    65.500 ms | table_ms    1.250, walk_ms   40.000 | sum   41.250 | 22 rounds, 6 groups'
    assert rt.mean_line('K13 pieces', 0.0655, acc, pr, with_sum=False) == \
        'K13 pieces             wall    65.500 ms | table_ms    1.250, walk_ms   40.000 | 22 rounds, 6 groups'
    assert rt.min_med_max([3e-3, 1e-3, 2e-3, 5e-3], 1e6) == '    1000.0 /     2500.0 /     5000.0 us'
    assert rt.mean_of([1.0, 2.0, 6.0]) == 1.0 / 3 + 2.0 / 3 + 6.0 / 3
