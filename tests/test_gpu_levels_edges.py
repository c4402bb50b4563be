"""xc_levels (k_levels) bit for bit against oracle.cal_contours and oracle.hist_edges at the level counts on both sides of its 256-thread
level loop, with many slabs of different ranges in one call, its `status` word, NaN and infinite extrema -- and xc_contours, whose
level kernel reduces K1's partials itself (the P > 0 path), against the bytes of xc_minmax followed by xc_levels."""
import warnings

import numpy as np
import pytest

import minmax_ref as M
import xcontour_oracle as O
from gpu_common import same_bits
from xcontour_amd import _native as nat

pytestmark = pytest.mark.gpu

NS = (2, 3, 255, 256, 257, 513, 1000)
RULES = ((nat.XC_EDGE_NUMPY, 'numpy'), (nat.XC_EDGE_XHISTOGRAM, 'xhistogram'))


def ranges(dt):
    """(rows of (min, max) in the tracer dtype, the rows whose extrema are infinite)"""
    rng = np.random.default_rng(20)
    fi = np.finfo(dt)
    rows = [(-1.5, 2.25), (1e-3, 1e3), (-7e5, -3.25), (0.0, float(fi.tiny)), (-float(fi.max) / 4, float(fi.max) / 4)]
    rows += [tuple(sorted(rng.standard_normal(2) * 10.0 ** e)) for e in (-20, -3, 0, 6, 30)]
    rows += [(2.5, 2.5), (0.0, 0.0)]                             # min == max
    rows += [(1.0, 1.0 + 3 * float(fi.eps)), (1.0, 1.0 + 3 * 2.0 ** -23), (-4.0 - 40 * 2.0 ** -21, -4.0)]      # a few ulps wide
    rows += [(np.nan, np.nan)]
    ninf = len(rows)
    rows += [(-np.inf, 1.0), (1.0, np.inf), (-np.inf, np.inf), (np.inf, np.inf), (-float(fi.max), float(fi.max))]
    return np.array(rows, dtype=dt), list(range(ninf, len(rows)))


def oracle_levels(mm, s, N, inc, cd):
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        return O.cal_contours(mm[s].reshape(1, 2), N, inc, cd)


def oracle_edges(ref, rule):
    with np.errstate(all='ignore'):
        e, _ = O.hist_edges(ref)
        if rule == 'xhistogram':
            e = np.concatenate((e[:-1], e[-1:] + 1e-8))
    return e.astype(np.float64)


@pytest.mark.parametrize('N', NS)
@pytest.mark.parametrize('dt', [np.float32, np.float64], ids=['q32', 'q64'])
def test_levels_edges_and_status_of_many_ranges_in_one_call(ctx, dt, N):
    """One call per (direction, contour dtype, right-edge rule) over ~20 slabs.  Levels: the oracle's, bit for bit, NaN where it has
    NaN.  status: 1 exactly where two neighbouring levels of the oracle are equal (min == max; a float32 contour over a range of a
    few ulps; infinite levels), 0 elsewhere in the same call -- a NaN never equals its neighbour, so an all-NaN slab says 0.  Edges:
    the oracle's hist_edges wherever it gives any (it raises on repeated levels).

    Infinite extrema: the levels and status agree with the oracle in every case here (inf * 0 = NaN at level 0, the rest infinite
    or NaN; asserted).  The edges are asserted too, except where the two rules differ by construction (read from both, not measured):
    hist_edges takes the direction from `b[0] < b[-1]`, which is False for a NaN end level
    whatever the direction was, while the kernel is told `increase`: an ascending [NaN, inf] (N = 2 over (1, inf)) is laid out
    [NaN, NaN, inf] by the kernel and [NaN, inf, NaN] by the oracle.  Neither is usable (the histogram refuses such edges), so
    the edges are compared where both end levels are numbers, or every level is NaN."""
    mm, infinite = ranges(dt)
    nslab = mm.shape[0]
    seen = {0: 0, 1: 0}
    for inc in (True, False):
        for cd in (np.float32, np.float64):
            for re_, rule in RULES:
                ctr, edges, st = ctx.levels(mm.astype(np.float64), dt, N, inc, cd, re_)
                assert ctr.shape == (nslab, N) and edges.shape == (nslab, N + 1) and st.shape == (nslab,)
                for s in range(nslab):
                    what = 'N %d %s q %s ctr %s %s slab %d %r' % (N, 'up' if inc else 'down', np.dtype(dt).name, np.dtype(cd).name, rule, s, mm[s].tolist())
                    ref = oracle_levels(mm, s, N, inc, cd)
                    same_bits(ctr[s], ref.astype(np.float64), what + ' levels')
                    repeated = bool((ref[1:] == ref[:-1]).any())
                    assert st[s] == (1 if repeated else 0), what + ' status %d' % st[s]
                    seen[int(repeated)] += 1
                    if s not in infinite and mm[s, 0] == mm[s, 1]:
                        assert repeated, what
                    ends_ok = not (np.isnan(ref[0]) or np.isnan(ref[-1])) or np.isnan(ref).all()
                    if not repeated and ends_ok:
                        same_bits(edges[s], oracle_edges(ref, rule), what + ' edges')
    assert seen[0] > 8 * 10 and seen[1] >= 8 * 2
    if N >= 255:                                                              # float32 contours over a few ulps repeat; float64 ones do not
        few = [s for s in range(nslab) if mm[s, 0] == 1.0 and mm[s, 1] == 1.0 + 3 * 2.0 ** -23]
        assert few
        for s in few:
            assert ctx.levels(mm.astype(np.float64), dt, N, True, np.float32)[2][s] == 1
            if dt is np.float64:
                assert ctx.levels(mm.astype(np.float64), dt, N, True, np.float64)[2][s] == 0


def contours_call(ctx, q, N, inc, cd, re_):
    """xc_contours with all four outputs"""
    nslab = q.shape[0]
    mm, ctr = np.empty((nslab, 2)), np.empty((nslab, N))
    edges, st = np.empty((nslab, N + 1)), np.empty(nslab, dtype=np.int32)
    ctx._check(ctx.lib.xc_contours(ctx.handle, nat._ptr(q), nat.dtype_code(q.dtype), nslab, q.size // nslab, N, int(inc), nat.dtype_code(cd),
                                   re_, nat._ptr(mm), nat._ptr(ctr), nat._ptr(edges), nat._ptr(st)))
    return mm, ctr, edges, st


@pytest.mark.parametrize('dt', [np.float32, np.float64], ids=['q32', 'q64'])
@pytest.mark.parametrize('nslab,ncell', [M.MANY_BLOCKS, (3, 4001)], ids=['P301', 'P1'])
def test_contours_in_one_call_with_many_partials(ctx, dt, nslab, ncell):
    """the level kernel's own reduction of K1's partials (P = 301: a second step of its 256-thread loop; P = 1): min / max, levels,
    edges and status are the bytes of xc_minmax followed by xc_levels.  The extrema sit in blocks 256 and 300, which only the second
    step reads; one slab of the small stack is constant (status 1) and one holds a NaN"""
    P = M.minmax_blocks(ncell, nslab)
    assert P == (301 if ncell > 10 ** 6 else 1)
    rng = np.random.default_rng(ncell)
    q = (rng.random((nslab, ncell)) * 1.98 - 0.99).astype(dt)
    if P == 301:
        p = M.Partition(np.dtype(dt).itemsize, ncell, nslab, 0, 0)
        mid = lambda b: p.cell((p.blocks[b][0] + p.blocks[b][1]) // 2, 0)
        q[0, mid(300)], q[0, mid(256)] = 3.0, -2.0
        q[1, mid(256)], q[1, mid(300)] = 5.0, -7.0
    else:
        q[1] = 0.25
        q[2, 17] = np.nan
    mm = ctx.minmax(q)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        assert np.array_equal(mm, np.stack([np.nanmin(q, axis=1), np.nanmax(q, axis=1)], axis=1).astype(np.float64))
    if P == 301:
        assert mm.tolist() == [[-2.0, 3.0], [-7.0, 5.0]]
    for N in (2, 257):
        for inc in (True, False):
            for cd in (np.float32, np.float64):
                for re_, _ in RULES:
                    one = contours_call(ctx, q, N, inc, cd, re_)
                    two = (mm,) + ctx.levels(mm, dt, N, inc, cd, re_)
                    for name, a, b in zip(('minmax', 'levels', 'edges', 'status'), one, two):
                        assert a.tobytes() == b.tobytes(), (name, N, inc, cd, re_)
                    if P == 1:
                        assert one[3].tolist() == [0, 1, 0]
