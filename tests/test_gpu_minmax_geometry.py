"""xc_minmax_dev (K1: k_minmax_partial + k_minmax_final) pinned by POSITION: for float32 and float64 stacks at every misalignment of the
call's pointer, every slab is a background in (-1, 1) whose maximum and minimum are planted at the position classes of minmax_ref.py
(every head and tail cell, the ends of the first / a middle / the last block, the load slots of the unrolled batch, the ends of the
remainder loop, both sides of every block cut), rotating over the slabs.  The reference is np.nanmin / np.nanmax of the slab; the
comparison is `==` on the values (both zeros are equal), NaN where the reference is NaN.  The shapes are minmax_ref.SHAPES, the smallest
that reach each regime (test_minmax_ref_host.py holds the proof).  Then the value classes (NaN beside the extremum, a vector of NaN,
an all-NaN slab, infinities, denormals, the largest finite number), the streaming-load instantiation in a child process with
XC_K1_NT=1 on the bytes of the parent, and the finite-only instantiation through the deterministic histogram."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import minmax_ref as M
from gpu_common import ROOT, _clean_env, bits
from xcontour_amd import _native as nat

pytestmark = pytest.mark.gpu

DT = {'f32': np.float32, 'f64': np.float64}
GUARD = 8
PATTERN = -1.2345e300


class Stack(object):
    """a background stack on the host and on the device, with room for every misalignment: the call at misalignment `mis` sees the
    elements [mis, mis + nslab * ncell) of one buffer that starts on a 16-byte boundary.  poke() writes the host and the device copy."""

    def __init__(self, ctx, dtname, nslab, ncell, seed):
        self.ctx, self.dt, self.nslab, self.ncell = ctx, np.dtype(DT[dtname]), nslab, ncell
        rng = np.random.default_rng(seed)
        n = nslab * ncell + 16 // self.dt.itemsize
        self.clean = (rng.random(n) * 1.98 - 0.99).astype(self.dt)
        assert np.abs(self.clean).max() < 1
        self.host = self.clean.copy()
        self.buf = ctx.to_device(self.host)
        assert self.buf.ptr % 16 == 0
        self.out = ctx.alloc((nslab + 2 * GUARD) * 16)
        self.poked = []

    def free(self):
        self.buf.free()
        self.out.free()

    def view(self, mis):
        return self.host[mis:mis + self.nslab * self.ncell].reshape(self.nslab, self.ncell)

    def poke(self, mis, s, cell, values):
        """cells [cell, cell + len(values)) of slab s of the call at `mis`"""
        values = np.atleast_1d(np.asarray(values, dtype=self.dt))
        assert 0 <= cell and cell + values.size <= self.ncell and 0 <= s < self.nslab
        e0 = mis + s * self.ncell + cell
        self.host[e0:e0 + values.size] = values
        self.ctx._check(self.ctx.lib.xc_memcpy_h2d(self.ctx.handle, self.buf.ptr + e0 * self.dt.itemsize, nat._ptr(values), values.nbytes))
        self.poked.append((e0, values.size))

    def restore(self):
        for e0, n in self.poked:
            self.host[e0:e0 + n] = self.clean[e0:e0 + n]
            part = np.ascontiguousarray(self.clean[e0:e0 + n])
            self.ctx._check(self.ctx.lib.xc_memcpy_h2d(self.ctx.handle, self.buf.ptr + e0 * self.dt.itemsize, nat._ptr(part), part.nbytes))
        self.poked = []

    def minmax(self, mis):
        """one xc_minmax_dev call on the misaligned pointer -> (nslab, 2); the words around the result stay as they were"""
        fill = np.full((self.nslab + 2 * GUARD) * 2, PATTERN)
        self.out.upload(fill)
        rc = self.ctx.lib.xc_minmax_dev(self.ctx.handle, self.buf.ptr + mis * self.dt.itemsize, nat.dtype_code(self.dt), self.nslab,
                                        self.ncell, self.out.ptr + GUARD * 16)
        assert rc == 0, 'xc_minmax_dev returned %d' % rc
        back = self.out.download(fill.shape, np.float64)
        assert (back[:2 * GUARD] == PATTERN).all() and (back[-2 * GUARD:] == PATTERN).all(), 'a word beside the result was written'
        return back[2 * GUARD:-2 * GUARD].reshape(self.nslab, 2)

    def reference(self, mis):
        v = self.view(mis)
        with np.errstate(all='ignore'):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)               # (an all-NaN slab: NaN, as the kernel must say)
                return np.stack([np.nanmin(v, axis=1), np.nanmax(v, axis=1)], axis=1).astype(np.float64)

    def check(self, mis, what):
        """the call against numpy -> the call's result.  `what(s)`: what was planted in slab s, for the message"""
        got, ref = self.minmax(mis), self.reference(mis)
        ok = (got == ref) | (np.isnan(got) & np.isnan(ref))
        if not ok.all():
            s, k = [int(i) for i in np.argwhere(~ok)[0]]
            raise AssertionError('%s %d x %d, pointer %d elements off, slab %d: %s is %r, numpy says %r (%d of %d values differ); planted: %s'
                                 % (self.dt.name, self.nslab, self.ncell, mis, s, ('min', 'max')[k], float(got[s, k]), float(ref[s, k]),
                                    int((~ok).sum()), ok.size, what(s)))
        return got


def run_positions(ctx, dtname, nslab, ncell, mis_list=None, record=None):
    """every position class of every slab carries the maximum once and the minimum once; -> the number of calls made"""
    st = Stack(ctx, dtname, nslab, ncell, seed=ncell)
    ncall = 0
    try:
        for mis in (M.misalignments(st.dt.itemsize) if mis_list is None else mis_list):
            per_slab = M.launch_classes(st.dt.itemsize, ncell, nslab, mis)
            for c, call in enumerate(M.schedule(per_slab)):
                for s, (a, b) in enumerate(call):
                    if a is not None:
                        st.poke(mis, s, per_slab[s][a], 2.0 + (per_slab[s][a] % 64) / 64.0)
                    if b is not None:
                        st.poke(mis, s, per_slab[s][b], -2.0 - (per_slab[s][b] % 64) / 64.0)
                got = st.check(mis, lambda s: 'max at %r, min at %r' % call[s])
                if record is not None:
                    record['pos_%s_%d_%d_%d_%d' % (dtname, nslab, ncell, mis, c)] = got
                st.restore()
                ncall += 1
    finally:
        st.free()
    return ncall


# ------------------------------------------------------------------ position classes
@pytest.mark.parametrize('nslab,ncell', [s for s in M.SHAPES if s != M.MANY_BLOCKS], ids=lambda v: str(v))
@pytest.mark.parametrize('dtname', ['f32', 'f64'])
def test_extrema_at_every_position_class(ctx, dtname, nslab, ncell):
    ncall = run_positions(ctx, dtname, nslab, ncell)
    if nslab == 700:
        assert ncall == 16 // np.dtype(DT[dtname]).itemsize, 'one call per misalignment covers all classes'


@pytest.mark.parametrize('dtname,mis', [('f32', 0), ('f32', 1), ('f32', 2), ('f32', 3), ('f64', 0), ('f64', 1)])
def test_extrema_on_both_sides_of_every_cut_of_301_blocks(ctx, dtname, mis):
    """P = 301: the 600 cut classes need some 300 calls of the two slabs; the stack is uploaded once and poked"""
    nslab, ncell = M.MANY_BLOCKS
    assert run_positions(ctx, dtname, nslab, ncell, [mis]) >= 300


@pytest.mark.parametrize('dtname', ['f32', 'f64'])
def test_final_reduction_takes_a_second_step_over_301_partials(ctx, dtname):
    """k_minmax_final walks the P partials 256 at a time: the extremum of a slab in the middle of block 0, 255, 256 and 300 in turn
    (threads 0, 255, 0 and 44, the last two in the second step), the maximum in one slab and the minimum in the other, then swapped"""
    nslab, ncell = M.MANY_BLOCKS
    st = Stack(ctx, dtname, nslab, ncell, seed=301)
    try:
        for mis in (0, 16 // st.dt.itemsize - 1):
            parts = [M.Partition(st.dt.itemsize, ncell, nslab, mis, s) for s in range(nslab)]
            assert all(p.P == 301 for p in parts)
            for blk in M.FINAL_BLOCKS:
                for flip in (0, 1):
                    for s, p in enumerate(parts):
                        v0, v1 = p.blocks[blk]
                        st.poke(mis, s, p.cell((v0 + v1) // 2, 1), 5.0 if (s + flip) % 2 == 0 else -5.0)
                    got = st.check(mis, lambda s: 'the extremum in block %d' % blk)
                    assert sorted(np.abs(got).max(axis=1).tolist()) == [5.0, 5.0]
                    st.restore()
    finally:
        st.free()


# ------------------------------------------------------------------ value classes
VAL_SHAPE = (4, 16381)                                                        # P = 4; odd: the slabs of one call differ in alignment
VAL_MIS = 1


def where(dt, mis=VAL_MIS):
    """{'head' / 'body' / 'tail': (slab, cell, partition)} of the value stack: a head cell, the last cell before a block cut, a tail cell"""
    nslab, ncell = VAL_SHAPE
    parts = [M.Partition(np.dtype(dt).itemsize, ncell, nslab, mis, s) for s in range(nslab)]
    assert all(p.P == 4 for p in parts)
    sh = next(s for s, p in enumerate(parts) if p.head > 0)
    stl = next(s for s, p in enumerate(parts) if p.tail[1] > p.tail[0])
    return {'head': (sh, parts[sh].head - 1, parts[sh]), 'body': (2, parts[2].cell(parts[2].blocks[2][0] - 1, parts[2].vn - 1), parts[2]),
            'tail': (stl, parts[stl].tail[0], parts[stl])}


def run_values(ctx, dtname, record=None):
    nslab, ncell = VAL_SHAPE
    st = Stack(ctx, dtname, nslab, ncell, seed=77)
    dt, mis = st.dt.type, VAL_MIS
    fi = np.finfo(dt)
    spots = where(dt)
    n = [0]

    def done(label):
        got = st.check(mis, lambda s: label)
        if record is not None:
            record['val_%s_%d' % (dtname, n[0])] = got
        n[0] += 1
        st.restore()
        return got

    def region(kind, s, cell, p):
        """the cells that share the load of `cell`: its vector, or the head / tail it lies in"""
        if kind == 'head':
            return 0, p.head
        if kind == 'tail':
            return p.tail
        v = (cell - p.head) // p.vn
        return p.cell(v, 0), p.cell(v + 1, 0)

    try:
        for kind, (s, cell, p) in spots.items():
            r0, r1 = region(kind, s, cell, p)
            for sign in (1.0, -1.0):
                # NaN in every other cell of the same load (the same float32 vector): the extremum beside them still counts
                row = np.full(r1 - r0, np.nan)
                row[cell - r0] = 3.0 * sign
                st.poke(mis, s, r0, row)
                got = done('%g among NaN in the %s' % (3.0 * sign, kind))
                assert got[s, 0 if sign < 0 else 1] == 3.0 * sign
                # infinities are extrema
                st.poke(mis, s, cell, sign * np.inf)
                got = done('%g in the %s' % (sign * np.inf, kind))
                assert got[s, 0 if sign < 0 else 1] == sign * np.inf
                # the largest finite number
                st.poke(mis, s, cell, sign * fi.max)
                got = done('%g in the %s' % (sign * fi.max, kind))
                assert got[s, 0 if sign < 0 else 1] == sign * float(fi.max)
                # denormals: a slab of one sign away from zero, the extremum the smallest denormal of that sign
                tiny = dt(fi.smallest_subnormal)
                assert 0 < float(tiny) < float(fi.tiny)
                v = st.view(mis)[s]
                st.poke(mis, s, 0, -sign * (np.abs(v) + dt(0.5)))
                st.poke(mis, s, cell, -sign * tiny)
                got = done('the denormal %g in the %s' % (-sign * float(tiny), kind))
                assert got[s, 1 if sign > 0 else 0] == -sign * float(tiny) and got[s, 1 if sign > 0 else 0] != 0.0
            # a load of nothing but NaN (a vector of four NaN; every head cell; every tail cell) beside an extremum the same thread reads
            st.poke(mis, s, r0, np.full(r1 - r0, np.nan))
            if kind == 'body':
                st.poke(mis, s, cell - 256 * p.vn, 4.0)
            got = done('only NaN in the %s' % kind)
            assert not np.isnan(got).any()
        # an all-NaN slab says NaN, NaN; its neighbours are not touched by it
        for s in (0, nslab - 1):
            st.poke(mis, s, 0, np.full(ncell, np.nan))
            got = done('slab %d all NaN' % s)
            assert np.isnan(got[s]).all() and not np.isnan(np.delete(got, s, axis=0)).any()
        for s in range(nslab):
            st.poke(mis, s, 0, np.full(ncell, np.nan))
        assert np.isnan(done('every slab all NaN')).all()
    finally:
        st.free()
    return n[0]


@pytest.mark.parametrize('dtname', ['f32', 'f64'])
def test_value_classes_in_a_head_a_body_and_a_tail_position(ctx, dtname):
    spots = where(DT[dtname])
    assert spots['head'][2].head > 0 and spots['tail'][2].tail[1] > spots['tail'][2].tail[0]
    assert run_values(ctx, dtname) == 3 * (2 * 4 + 1) + 3


# ------------------------------------------------------------------ the streaming loads (NT) in a child process
NT_SHAPES = M.SMALL + [M.ONE_BLOCK, M.SHORT_LAST]


def small_suite(ctx):
    """{key: (nslab, 2) result} of every call of the position classes on the small shapes and of the value classes, each checked
    against numpy on the way"""
    out = {}
    for dtname in ('f32', 'f64'):
        for nslab, ncell in NT_SHAPES:
            run_positions(ctx, dtname, nslab, ncell, record=out)
        run_values(ctx, dtname, record=out)
    return out


def run_child(path):
    """the child process of `streaming`: one context under XC_K1_NT=1"""
    assert os.environ.get('XC_K1_NT') == '1'
    ctx = nat.Context(0)
    try:
        np.savez(path, **small_suite(ctx))
    finally:
        ctx.close()


@pytest.fixture(scope='module')
def streaming(tmp_path_factory):
    """XC_K1_NT=1 in ONE child process with one context: k_minmax_partial<T, NT = true> on the small suite"""
    path = str(tmp_path_factory.mktemp('k1_nt') / 'out.npz')
    env = _clean_env()
    env['XC_K1_NT'] = '1'
    src = 'import sys; sys.path[:0] = [%r, %r, %r]\n' % (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')) \
        + 'import test_gpu_minmax_geometry as T\nT.run_child(%r)\nprint("OK")\n' % path
    p = subprocess.run([sys.executable, '-c', src], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert p.returncode == 0 and 'OK' in p.stdout, p.stdout[-3000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def test_streaming_loads_return_the_bytes_of_the_plain_loads(ctx, streaming):
    assert os.environ.get('XC_K1_NT', '0') == '0', 'the parent runs the plain loads'
    mine = small_suite(ctx)
    assert sorted(mine) == sorted(streaming) and len(mine) > 100
    for k in sorted(mine):
        a, b = mine[k], streaming[k]
        assert a.shape == b.shape and ((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all(), k


# ------------------------------------------------------------------ the finite-only instantiation (FIN), through the deterministic histogram
FIN_SHAPE = (4, 127, 129)                                                    # 16383 cells a slab: P = 4, and four alignments in one stack


@pytest.mark.parametrize('dtname', ['f32', 'f64'])
def test_finite_only_extrema_fix_the_windows_of_the_deterministic_sums(ctx, dtname):
    """k_minmax_partial<T, false, FIN = true> has no entry of its own: det_one_pass (xc_keff.hip) runs it over every integrand of
    ctx.hist(..., deterministic=True) and sets the window of that channel's fixed-point accumulators from the slab's largest finite
    magnitude (xc_binning.h det_c0_from_bound: 12 bits of slack above the bound, 180 bits below it).

    What a term above the window does, as read in xc_binning.h det_split and xc_hist_kernel.h: it is NOT flagged.  Only an infinite
    weight (exponent 0x7ff) sets the flag that makes k_det3_reduce report NaN for its bin.  A finite term up to 2^12 times the bound
    still lies inside the window and is summed correctly; a larger one has its chunks shifted by a count that is out of range and
    clamped into the cell's own limbs: the sum of its bin is silently wrong.  So the planted magnitude here is 2^40 times everything
    else: had K1 missed it, the window would sit 28 bits too low and the bin that holds it could not equal the exact sum.

    One integrand whose largest finite magnitude (+-2^40 among multiples of 2^-10 below 1) sits in turn in every cell that can be a
    head, a tail or a side of a block cut of its slab under any alignment of the staged stack; an infinity sits in a bin of its own.
    Every bin without the infinity equals math.fsum of its terms bit for bit; the bin with it is NaN."""
    dt = DT[dtname]
    nslab, ny, nx = FIN_SHAPE
    ncell = ny * nx
    assert M.minmax_blocks(ncell, nslab) == 4
    rng = np.random.default_rng(950)
    q = (np.arange(nslab * ncell) % 3 + 0.5).reshape(nslab, ny, nx)
    inf_cell = ncell // 2 + 5
    q.reshape(nslab, ncell)[:, inf_cell] = 3.5
    edges = np.arange(5.0)
    clean = (rng.integers(-1000, 1001, size=(nslab, ncell)) * 2.0 ** -10).astype(dt)
    cells = set()
    for mis in M.misalignments(np.dtype(dt).itemsize):
        for s in range(nslab):
            c = M.classes(M.Partition(np.dtype(dt).itemsize, ncell, nslab, mis, s))
            cells |= set(v for k, v in c.items() if k.startswith(('head', 'tail', 'cut')))
    cells = sorted(cells - {inf_cell})
    assert {0, ncell - 1} <= set(cells) and 8 <= len(cells) <= 80
    flat_q = q.reshape(nslab, ncell)
    for i, cell in enumerate(cells):
        f = clean.copy()
        for s in range(nslab):
            f[s, cells[(i + s) % len(cells)]] = (-1.0) ** s * 2.0 ** 40
            f[s, inf_cell] = (-1.0) ** (i + s) * np.inf
        out = ctx.hist(q, edges, integrands=[f.reshape(nslab, ny, nx)], want=('pdf', 'counts'), deterministic=True)
        for s in range(nslab):
            assert np.isnan(out['pdf'][s, 1, 3]) and out['counts'][s, 3] == 1, 'the bin of the infinity'
            for k in range(3):
                terms = f[s][flat_q[s] == k + 0.5].astype(np.float64)
                assert out['counts'][s, k] == terms.size
                want = math.fsum(terms.tolist())
                assert bits(out['pdf'][s, 1, k]) == bits(want), \
                    '%s slab %d bin %d with 2^40 at cell %d: %r, exactly %r' % (dtname, s, k, cells[(i + s) % len(cells)], float(out['pdf'][s, 1, k]), want)
                assert out['pdf'][s, 0, k] == terms.size
