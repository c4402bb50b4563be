"""-m gpu: the K7 band walk (k_lwa_strip; k_lwa_prep + k_lwa) at every staging chunk and every rank of the weight and the metric.

k_lwa_strip stages plane-rank weights and metrics 64, 32 or 16 rows at a time, whichever layout fits the LDS; row-rank ones are not
staged at all.  Which chunk a call took cannot be seen from outside, so every case here takes its plan from lwa_plan_ref.walk_plan
(pinned on a hand-worked table by test_lwa_plan_host.py) and asserts it -- and asserts through lwa_plan_ref.band, before the GPU is
asked, that its fields make the chunk loop do what the case is about: three or more chunks with a wave's band cut by a chunk boundary,
a workgroup whose union band is empty or fits one chunk, a wave whose band starts in a chunk other than the first.

Everything is compared bit for bit (np.array_equal, NaN equal to NaN) with the oracle's literal loop (core.py:752-791 / 858-897): no
tolerance anywhere.  The oracle wants 2-D weights: a row dA goes to it broadcast to the plane (dA / max is the same per cell).

Fields (`_case`, built like test_gpu_lwa._streaming_walk_case): two distinct slabs of ny x 130 (three strips, the last with two live columns), a meandering front on a gentle slope
plus noise, a whole row of NaN, a +inf and a -inf cell, a constant row, cells exactly on reference levels; slab 0 has a sorted Q (narrow
bands), slab 1 a Q that is not monotone (bands that span the plane).  Weights and metrics are random in [0.5, 1.5), constant along
neither axis: a wrong row or column index changes bits.
"""
import functools
import os
from concurrent.futures import ThreadPoolExecutor
import subprocess
import sys

import numpy as np
import pytest

import xcontour_oracle as O
import lwa_plan_ref as P
from gpu_common import ROOT, _clean_env

pytestmark = pytest.mark.gpu

NX = 130                                                  # three strips; two live columns in the last
PARTS = (('all', 0), ('upper', 1), ('lower', 2))
VI = [(0, True), (0, False), (1, True), (1, False)]       # (variant, increase): with the three parts, the 12 calls of a case
VI_IDS = ['lwa-inc', 'lwa-dec', 'lwa2-inc', 'lwa2-dec']
RANKS = [(da, m) for da in ('row', 'plane') for m in (None, 'row', 'plane')]
DT = {'f64': np.float64, 'f32': np.float32}


@functools.lru_cache(maxsize=None)
def _case(dtname, ny, kind='up'):
    """-> dict: coord (ny,), q (2, ny, NX) of the dtype, Q (2, ny), 'row' / 'plane' weights and metrics.  kind: 'up' an increasing
    coordinate, 'down' a decreasing one, 'tied' an increasing one with two equal neighbouring values inside the front"""
    dt = DT[dtname]
    rng = np.random.default_rng(7000 + ny)
    lat = np.linspace(-80, 80, ny)
    # the front: 2 degrees wide, meandering by 10 degrees along x; the slope keeps the rows apart where the front is flat (the noise is
    # a tenth of the slope's step per row at ny = 500), so that away from the front a sorted Q gives bands of a few rows
    front = np.tanh((lat[:, None] - 10 * np.sin(np.linspace(0, 6.28, NX))[None, :]) / 2.0) + 0.01 * lat[:, None]
    q = (front[None] + 3e-4 * rng.standard_normal((2, ny, NX))).astype(dt)
    Q0 = np.sort(q[0, :, 0].astype(np.float64))                                       # sorted: narrow bands
    Q1 = (0.8 * rng.standard_normal(ny)).astype(dt).astype(np.float64)                # not monotone: bands that span the plane
    # cells exactly ON reference levels: in slab 0 the level of a row on that row or a neighbour (it stays inside the band), in slab 1 anywhere
    jj, xx = rng.integers(1, ny - 1, 150), rng.integers(0, NX, 150)
    q[0, jj + rng.integers(-1, 2, 150), xx] = Q0[jj].astype(dt)
    q[1, rng.integers(0, ny, 150), rng.integers(0, NX, 150)] = Q1[rng.integers(0, ny, 150)].astype(dt)
    q[0, ny // 3, :] = np.nan                                                         # a whole row of NaN
    q[0, ny // 2, 2] = np.inf; q[1, 1, 1] = -np.inf
    q[1, ny // 4, :] = 0.25                                                           # a constant row
    Q = np.stack([Q0, Q1])
    assert min(int((q[s].astype(np.float64)[:, :, None] == Q[s][None, None, ::7]).sum()) for s in (0, 1)) >= 10
    coord = lat
    if kind == 'down':
        coord = lat[::-1].copy()
    elif kind == 'tied':
        coord = lat.copy(); coord[ny // 2 + 1] = coord[ny // 2]
        assert (np.diff(coord) == 0).sum() == 1
    w = {'row': rng.random(ny) + 0.5, 'plane': rng.random((ny, NX)) + 0.5}
    m = {'row': rng.random(ny) + 0.5, 'plane': rng.random((ny, NX)) + 0.5, None: None}
    for a in (q, Q, coord, *w.values(), m['row'], m['plane']):
        a.setflags(write=False)
    return {'coord': coord, 'q': q, 'Q': Q, 'w': w, 'm': m, 'dt': dtname, 'ny': ny, 'kind': kind}


_REFS = {}
_KEEP = set()             # (dtname, ny, kind, da, m): cases whose oracle planes a second test needs


def _refs(case, da, m, variant, increase):
    """the oracle's planes of the two slabs for each part -> {part code: [ref slab 0, ref slab 1]}; computed once for the cases in _KEEP"""
    key = (case['dt'], case['ny'], case['kind'], da, m, variant, increase)
    if key in _REFS:
        return _REFS[key]
    fn = O.cal_local_wave_activity2 if variant else O.cal_local_wave_activity
    dA = np.broadcast_to(case['w'][da][:, None], (case['ny'], NX)) if da == 'row' else case['w'][da]

    def plane(job):
        name, s = job
        with np.errstate(invalid='ignore'):                                           # inf * 0 inside the oracle's products
            return fn(case['q'][s].astype(np.float64), case['Q'][s], case['coord'], dA, increase, name, metric=case['m'][m])
    # one oracle plane is ny small numpy steps, which release the interpreter lock: the six planes side by side
    with ThreadPoolExecutor(6) as ex:
        planes = list(ex.map(plane, [(name, s) for name, _ in PARTS for s in (0, 1)]))
    out = {pc: planes[2 * i:2 * i + 2] for i, (_, pc) in enumerate(PARTS)}
    if key[:5] in _KEEP:
        _REFS[key] = out
    return out


@functools.lru_cache(maxsize=None)
def _premises(dtname, ny, kind, wchunk):
    """the three premises on the fields of a case staged `wchunk` rows at a time, over its 12 calls, both slabs and the three strips ->
    (a workgroup -- 8 consecutive target rows of one strip -- with a union band of more than 2 wchunk rows, so three or more chunks, and
    a wave's band cut by a chunk boundary; a workgroup whose union band is empty or fits one chunk; a wave whose band starts in a chunk
    other than the first)"""
    case = _case(dtname, ny, kind)
    wide = narrow = late = False
    for variant, increase in VI:
        for _, pc in PARTS:
            for s in (0, 1):
                for strip in range((NX + 63) // 64):
                    y0, y1 = P.bands(case['q'][s], case['Q'][s], case['coord'], increase, pc, variant, strip)
                    for g in P.workgroups(y0, y1, wchunk):
                        span = g['union'][1] - g['union'][0]
                        wide |= span > 2 * wchunk and g['chunks'] >= 3 and g['cut']
                        narrow |= span <= wchunk
                        late |= g['late']
    return wide, narrow, late


def _run(ctx, case, da, m, variant, increase, idx=(0, 1), ref=None):
    """the three parts of (variant, increase) on the stack q[idx], each slab against the oracle of its distinct slab"""
    ref = _refs(case, da, m, variant, increase) if ref is None else ref
    idx = np.asarray(idx)
    dA, M = case['w'][da], case['m'][m]
    q, Q = np.ascontiguousarray(case['q'][idx]), np.ascontiguousarray(case['Q'][idx])
    for name, pc in PARTS:
        out, _ = ctx.lwa(q, Q, case['coord'], dA, float(dA.max()), M=M, increase=increase, part=pc, variant=variant)
        assert ctx.last_lwa_path() == 0
        for k, s in enumerate(idx):
            if not np.array_equal(out[k], ref[pc][s], equal_nan=True):
                bad = np.argwhere(~((out[k] == ref[pc][s]) | (np.isnan(out[k]) & np.isnan(ref[pc][s]))))
                raise AssertionError('%s ny=%d dA %s M %s variant %d increase %s part %s slab %d (of %d): %d cells differ, first at target row %d '
                                     'column %d: %r != %r (oracle)' % (case['dt'], case['ny'], da, m, variant, increase, name, s, len(idx),
                                                                       len(bad), bad[0][0], bad[0][1], out[k][tuple(bad[0])],
                                                                       ref[pc][s][tuple(bad[0])]))


def _tsize(dtname):
    return np.dtype(DT[dtname]).itemsize


# ---------------------------------------------------------------- a. the strip kernel: every chunk, every rank
def _strip_cases():
    out = []
    for dtname in ('f64', 'f32'):
        for da, m in RANKS:
            staged = any(P.planes(da, m))
            for target in ((64, 32, 16) if staged else ('none staged',)):
                plan = ('strip', target if staged else 64)
                out.append((dtname, da, m, target, P.largest_ny(plan, 2, NX, _tsize(dtname), da, m), plan))
    # both planes, one row past each limit: the next chunk at its loosest fit
    out += [('f64', 'plane', 'plane', 32, 155, ('strip', 32)), ('f64', 'plane', 'plane', 16, 213, ('strip', 16)),
            ('f32', 'plane', 'plane', 32, 286, ('strip', 32)), ('f32', 'plane', 'plane', 16, 393, ('strip', 16))]
    return out


STRIP_CASES = _strip_cases()
_KEEP |= {('f64', 241, 'up', 'plane', 'plane'), ('f32', 392, 'up', 'plane', 'plane')}        # section d runs these on the other kernel


def _strip_id(c):
    return '%s-dA_%s-M_%s-chunk_%s-ny%d' % (c[0], c[1], c[2], str(c[3]).replace(' ', '_'), c[4])


def test_strip_cases_sit_on_the_limits_of_the_plan():
    """the sizes the cases above take from walk_plan, against the limits worked out by hand in test_lwa_plan_host.py"""
    got = {(c[0], c[1], c[2], c[3]): c[4] for c in STRIP_CASES[:-4]}
    assert [got['f64', 'plane', 'plane', t] for t in (64, 32, 16)] == [154, 212, 241]
    assert [got['f32', 'plane', None, t] for t in (64, 32, 16)] == [285, 392, 445]
    assert [got['f64', 'row', 'plane', t] for t in (64, 32, 16)] == [212, 241, 255] == [got['f64', 'plane', 'row', t] for t in (64, 32, 16)]
    assert [got['f32', 'plane', 'row', t] for t in (64, 32, 16)] == [392, 445, 471] == [got['f32', 'row', 'plane', t] for t in (64, 32, 16)]
    assert got['f64', 'row', None, 'none staged'] == got['f64', 'row', 'row', 'none staged'] == 270
    assert got['f32', 'row', None, 'none staged'] == got['f32', 'row', 'row', 'none staged'] == 498
    assert len(STRIP_CASES) == 2 * (4 * 3 + 2) + 4
    for c in STRIP_CASES:
        # idle waves in the last workgroup (they still join the staging barriers) at every size but 392 = 49 * 8
        assert (c[4] % P.LWA_SW != 0) == (c[4] != 392)


@pytest.mark.parametrize('variant,increase', VI, ids=VI_IDS)
@pytest.mark.parametrize('dtname,da,m,target,ny,plan', STRIP_CASES, ids=[_strip_id(c) for c in STRIP_CASES])
def test_lwa_strip_every_chunk_and_rank(ctx, dtname, da, m, target, ny, plan, variant, increase):
    """k_lwa_strip at the tightest LDS fit of every staging chunk (and one row past the limits of 64 and 32: the loosest fit of the next),
    for the six rank combinations of weight and metric and both tracer types.  The chunk is walk_plan's; the premises on the fields are
    asserted before the GPU is asked (through bands, which test_lwa_plan_host.py holds equal to band row by row)."""
    assert P.walk_plan(2, ny, NX, _tsize(dtname), da, m) == plan
    if STRIP_CASES.index((dtname, da, m, target, ny, plan)) < len(STRIP_CASES) - 4:
        assert P.walk_plan(2, ny + 1, NX, _tsize(dtname), da, m) != plan               # the largest such ny
    else:
        assert P.walk_plan(2, ny - 1, NX, _tsize(dtname), da, m) == ('strip', 2 * target)      # one row past the limit of the chunk before
    case = _case(dtname, ny)
    if target != 'none staged':
        wide, narrow, late = _premises(dtname, ny, 'up', plan[1])
        assert wide, 'no workgroup with three or more chunks and a band cut by a chunk boundary'
        assert narrow, 'no workgroup whose union band is empty or fits one chunk'
        assert late, 'no wave whose band starts in a chunk other than the first'
    else:
        assert not any(P.planes(da, m))
    _run(ctx, case, da, m, variant, increase)


# ---------------------------------------------------------------- b. coordinate direction and ties
CHUNK_NY = {64: 154, 32: 212, 16: 241}                   # float64, both planes


@pytest.mark.parametrize('variant,increase', VI, ids=VI_IDS)
@pytest.mark.parametrize('kind', ['down', 'tied'])
@pytest.mark.parametrize('wchunk', [64, 32, 16])
def test_lwa_strip_coordinate_direction_and_ties(ctx, wchunk, kind, variant, increase):
    """a decreasing coordinate, and one with two equal neighbouring values inside the front (lwa_near is >= / <=, as the oracle's
    core.py:757 is: each of the two rows is on the near side of the other), at every chunk size; float64, weight and metric planes"""
    ny = CHUNK_NY[wchunk]
    assert P.walk_plan(2, ny, NX, 8, 'plane', 'plane') == ('strip', wchunk)
    case = _case('f64', ny, kind)
    d = np.diff(case['coord'])
    assert (d < 0).all() if kind == 'down' else ((d >= 0).all() and (d == 0).sum() == 1)
    wide, narrow, late = _premises('f64', ny, kind, wchunk)
    assert wide and narrow and late
    _run(ctx, case, 'plane', 'plane', variant, increase)


# ---------------------------------------------------------------- c. the streaming kernel just past the strip
@pytest.mark.parametrize('variant,increase', VI, ids=VI_IDS)
@pytest.mark.parametrize('da,m', RANKS, ids=['dA_%s-M_%s' % r for r in RANKS])
@pytest.mark.parametrize('dtname,ny', [('f64', 242), ('f32', 446)])
def test_lwa_streaming_walk_just_past_the_strip(ctx, dtname, ny, da, m, variant, increase):
    """the first plane height whose strip no longer fits with both planes: k_lwa_prep + k_lwa under default knobs, for the six rank
    combinations, with one target row per thread (k_lwa<.., 1>) and with four (k_lwa<.., 4>: the same two slabs repeated to the smallest
    stack with ny^2 nx nslab >= 2e8).  With both planes a stack of two slabs streams.  With one plane or none the strip still fits at
    this height (its limits are 255 / 270 rows in float64, 471 / 498 in float32), so two slabs would take k_lwa_strip: there the
    one-target stack is the smallest that leaves `few` (6 slabs of 242 rows, 4 of 446) -- walk_plan says so on both sides of each."""
    ts = _tsize(dtname)
    assert P.walk_plan(2, ny, NX, ts, 'plane', 'plane') == ('stream', 1) and P.walk_plan(2, ny - 1, NX, ts, 'plane', 'plane') == ('strip', 16)
    S1 = max(2, P.smallest_stack(('stream', 1), ny, NX, ts, da, m))              # two distinct slabs at the least
    S4 = P.smallest_stack(('stream', 4), ny, NX, ts, da, m)
    assert S1 == (2 if all(P.planes(da, m)) else {242: 6, 446: 4}[ny]) and S4 == {242: 27, 446: 8}[ny]
    assert P.walk_plan(S1, ny, NX, ts, da, m) == ('stream', 1) and (S1 == 2 or P.walk_plan(S1 - 1, ny, NX, ts, da, m)[0] == 'strip')
    assert P.walk_plan(S4 - 1, ny, NX, ts, da, m) == ('stream', 1) and float(ny) ** 2 * NX * (S4 - 1) < 2.0e8 <= float(ny) ** 2 * NX * S4
    case = _case(dtname, ny)
    ref = _refs(case, da, m, variant, increase)
    _run(ctx, case, da, m, variant, increase, idx=np.arange(S1) % 2, ref=ref)
    _run(ctx, case, da, m, variant, increase, idx=np.arange(S4) % 2, ref=ref)


# ---------------------------------------------------------------- d. one kernel against the other
OTHER = [('f64', 241, 16), ('f32', 392, 32)]             # (dtype, ny, the chunk k_lwa_strip stages them with), weight and metric planes


def run_other_kernel(ctx, path):
    """the child process of `other_kernel`: the 12 calls of each OTHER case, saved for the parent"""
    out = {}
    for dtname, ny, _ in OTHER:
        case = _case(dtname, ny)
        dA, M = case['w']['plane'], case['m']['plane']
        for variant, increase in VI:
            for _, pc in PARTS:
                got, _ = ctx.lwa(case['q'], case['Q'], case['coord'], dA, float(dA.max()), M=M, increase=increase, part=pc, variant=variant)
                assert ctx.last_lwa_path() == 0
                out['%s_%d_%d_%d' % (dtname, variant, int(increase), pc)] = got
    np.savez(path, **out)


@pytest.fixture(scope='module')
def other_kernel(tmp_path_factory):
    """XC_LWA_STRIP=0 in ONE child process with one context: the OTHER cases on k_lwa_prep + k_lwa"""
    for dtname, ny, wchunk in OTHER:
        assert P.walk_plan(2, ny, NX, _tsize(dtname), 'plane', 'plane') == ('strip', wchunk)
        assert P.walk_plan(2, ny, NX, _tsize(dtname), 'plane', 'plane', knob_strip=0) == ('stream', 1)
    path = str(tmp_path_factory.mktemp('lwa_other') / 'out.npz')
    env = _clean_env()
    env['XC_LWA_STRIP'] = '0'
    src = 'import sys; sys.path[:0] = [%r, %r, %r]\n' % (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')) \
        + 'import test_gpu_lwa_walk as T\nfrom xcontour_amd import _native as nat\nctx = nat.Context(0)\nT.run_other_kernel(ctx, %r)\nctx.close()\nprint("OK")\n' % path
    p = subprocess.run([sys.executable, '-c', src], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert p.returncode == 0 and 'OK' in p.stdout, p.stdout[-3000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize('variant,increase', VI, ids=VI_IDS)
@pytest.mark.parametrize('dtname,ny,wchunk', OTHER, ids=['%s-ny%d-chunk%d' % c for c in OTHER])
def test_lwa_streaming_kernel_on_the_strip_kernels_cases(other_kernel, dtname, ny, wchunk, variant, increase):
    """the float64 chunk-16 and the float32 chunk-32 cases of test_lwa_strip_every_chunk_and_rank on the streaming kernel: with that test
    both kernels are pinned on the same bits (the oracle's planes are computed once for both)"""
    ref = _refs(_case(dtname, ny), 'plane', 'plane', variant, increase)
    for name, pc in PARTS:
        got = other_kernel['%s_%d_%d_%d' % (dtname, variant, int(increase), pc)]
        for s in (0, 1):
            assert np.array_equal(got[s], ref[pc][s], equal_nan=True), (dtname, variant, increase, name, s)


# ---------------------------------------------------------------- e. the facade at the two reanalysis grids
def _grid_case(ny, nx):
    rng = np.random.default_rng(ny)
    lat, lon = np.linspace(-90, 90, ny), np.arange(nx) * (360.0 / nx)
    q = np.tanh((lat[:, None] - 12 * np.sin(np.deg2rad(3 * lon))[None, :]) / 6.0) + 0.005 * lat[:, None] + 0.01 * rng.standard_normal((ny, nx))
    q[ny // 5, 7:40] = np.nan
    Q = np.sort(q[:, 0])
    dA2 = O.cell_area(lat, lon) * (0.9 + 0.2 * rng.random((ny, nx)))                  # not constant along x
    dy = np.abs(np.gradient(np.deg2rad(lat))) * O.Rearth * (0.9 + 0.2 * rng.random(ny))
    return lat, lon, q, Q, dA2, dy


@pytest.mark.parametrize('ny,nx,da_rank,wchunk', [(181, 360, 'plane', 32), (241, 480, 'plane', 16), (241, 480, 'row', None)],
                         ids=['1deg', '0.75deg', '0.75deg-dA_1d'])
def test_facade_lwa_and_lape_at_the_reanalysis_grids(ny, nx, da_rank, wchunk):
    """Contour2D.cal_local_wave_activity / cal_local_APE on a 1 degree and a 0.75 degree global grid in float64.  With the default metric
    (M = dA, a plane) the first is staged 32 rows at a time and the second, one row under the limit, 16; part='upper' with a row metric
    leaves one plane (chunk 64 at 181 rows, 32 at 241), and a 1-D dA with it none.  All against the oracle, bit for bit."""
    import xcontour_amd as xa
    lat, lon, q, Q, dA2, dy = _grid_case(ny, nx)
    c = {'lat': lat, 'lon': lon}
    tr = xa.DataArray(q, ('lat', 'lon'), c, 'pv')
    dAv = dA2 if da_rank == 'plane' else dA2[:, 0].copy()
    dA = xa.DataArray(dAv, ('lat', 'lon') if da_rank == 'plane' else ('lat',), c if da_rank == 'plane' else {'lat': lat}, 'dA')
    dAo = dA2 if da_rank == 'plane' else np.broadcast_to(dAv[:, None], (ny, nx))
    Qd = xa.DataArray(Q, ('lat',), {'lat': lat}, 'pv')
    assert P.walk_plan(1, ny, nx, 8, da_rank, None) == ('strip', wchunk if wchunk else 64) and any(P.planes(da_rank, None)) == bool(wchunk)
    assert P.walk_plan(1, ny, nx, 8, da_rank, 'row') == ('strip', 32 if (ny, da_rank) == (241, 'plane') else 64)
    cm = xa.Contour2D(tr, dA, dims={'X': 'lon', 'Y': 'lat'}, dimEq={'Y': 'lat'}, increase=True, lt=True)
    try:
        for kw, okw in (({}, {}), ({'part': 'upper', 'metric': dy}, {'metric': dy})):
            ref = O.cal_local_wave_activity(q, Q, lat, dAo, True, kw.get('part', 'all'), **okw)
            assert np.isfinite(ref).all() and np.abs(ref).max() > 0
            lwa = cm.cal_local_wave_activity(tr, Qd, **kw)
            assert cm.ctx.last_lwa_path() == 0 and lwa.dims == tr.dims
            assert np.array_equal(lwa.values, ref, equal_nan=True), kw
            ape = cm.cal_local_APE(tr, Qd, **kw)
            assert cm.ctx.last_lwa_path() == 0 and ape.name == 'LAPE'
            assert np.array_equal(ape.values, ref, equal_nan=True), kw
    finally:
        cm.close()
