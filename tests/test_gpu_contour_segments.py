"""K12 (xc_contour_segments, Context.contour_segments) on the GPU against the restatement contour_join_ref: after the sort by
e_from inside every range, counts, edge ids and end points are EQUAL -- the end points bit for bit."""
import numpy as np
import pytest

import contour_join_ref as JR
from xcontour_amd import _native as nat

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_records(got, ref, what=''):
    assert np.array_equal(got[0].astype(np.int64), ref[0].astype(np.int64)), what + ': counts'
    assert np.array_equal(got[1], ref[1]), what + ': e_from'
    assert np.array_equal(got[2], ref[2]), what + ': e_to'
    assert got[3].shape == ref[3].shape and np.array_equal(bits(got[3]), bits(ref[3])), what + ': pts'


def check(ctx, q, lv, what=''):
    got = ctx.contour_segments(q, lv)
    assert got[0].dtype == np.uint64 and got[1].dtype == np.int64 and got[2].dtype == np.int64 and got[3].dtype == np.float64
    same_records(got, JR.stack_records(q.astype(np.float64), lv), what)
    return got


def field(kind, shape, seed=7):
    rng = np.random.default_rng(seed)
    if kind == 'saddle':
        return np.indices(shape[-2:]).sum(0) % 2 * 2.0 - 1.0 + 0.3 * rng.standard_normal(shape)       # checkerboard
    q = rng.standard_normal(shape)
    if kind == 'nan':
        q[rng.random(shape) < 0.03] = np.nan
    return q


@pytest.mark.parametrize('kind', ['random', 'saddle', 'nan'])
@pytest.mark.parametrize('dt', [np.float32, np.float64])
def test_matches_restatement(ctx, kind, dt):
    """3 slabs of 70 x 520: three tile rows and three tile columns, the last of each partial"""
    q = field(kind, (3, 70, 520)).astype(dt)
    lv = np.linspace(-2.0, 2.0, 37)
    got = check(ctx, q, lv, kind + ' shared')
    assert got[0].sum() > 10000
    check(ctx, q, lv[None, :] + 0.013 * np.arange(3)[:, None], kind + ' per slab')


@pytest.mark.parametrize('shape', [(1, 2, 2), (1, 33, 253), (1, 34, 254), (2, 1, 9), (2, 9, 1)])
@pytest.mark.parametrize('dt', [np.float32, np.float64])
def test_shapes_at_the_tile_seams(ctx, shape, dt):
    q = field('random', shape, seed=3).astype(dt)
    got = check(ctx, q, np.array([-0.7, 0.0, 0.4]), str(shape))
    if min(shape[1:]) < 2:
        assert got[0].sum() == 0 and got[1].size == 0 and got[3].shape == (0, 4)        # no cells


def test_empty_ranges_and_a_nan_slab(ctx):
    rng = np.random.default_rng(5)
    q = rng.random((3, 40, 300))
    q[:, :, 150:] += 3.0                                  # columns 0..149 in [0, 1), 151.. in [3, 4)
    q[:, :, 150] = np.nan                                 # and nothing joins the two: a level between them crosses no cell
    q[1] = np.nan                                         # a slab that is entirely NaN
    lv = np.array([-2.0, -1.0, 0.5, 2.0, 3.5, 7.0, 8.0])
    got = check(ctx, q, lv)
    c = got[0].astype(np.int64)
    assert (c[1] == 0).all() and (c[[0, 2]][:, [0, 1, 3, 5, 6]] == 0).all() and (c[[0, 2]][:, [2, 4]] > 0).all()


def test_more_levels_than_one_group_and_a_single_level(ctx):
    q = field('random', (2, 9, 70), seed=9)
    N = nat.XC_CSEG_GROUP_LEVELS + 3
    lv = np.sort(np.random.default_rng(1).uniform(-2.5, 2.5, N))
    check(ctx, q, lv, 'N = %d' % N)
    check(ctx, q, np.linspace(-2.5, 2.5, N), 'N = %d equally spaced' % N)
    check(ctx, q, np.array([0.1]), 'N = 1')


def test_many_blocks_per_slab_and_many_slabs(ctx):
    lv = np.array([-1.0, -0.2, 0.0, 0.3, 1.1])
    big = field('nan', (1, 200, 1100), seed=2)            # 35 tiles, one block each
    one = check(ctx, big, lv, 'one large slab')
    small = field('random', (40, 20, 60), seed=4)         # 40 slabs of one tile
    check(ctx, small, lv, 'forty slabs')
    # the same plane alone and inside a stack: the same records
    stack = field('random', (5, 200, 1100), seed=6)
    stack[3] = big[0]
    got = ctx.contour_segments(stack, lv)
    off = np.concatenate([[0], np.cumsum(got[0].ravel().astype(np.int64))])
    a, b = off[3 * lv.size], off[4 * lv.size]
    same_records((got[0][3:4], got[1][a:b], got[2][a:b], got[3][a:b]), one, 'alone against inside a stack')


def test_capacity_protocol(ctx):
    q = field('random', (2, 30, 90), seed=8)
    lv = np.array([-0.5, 0.0, 0.5])
    ref = JR.stack_records(q, lv)
    total = int(ref[0].sum())
    lib, f64 = ctx.lib, nat.XC_F64
    dq, dc, dn = ctx.to_device(q), ctx.to_device(lv), ctx.alloc(2 * 3 * 8)
    head = (ctx.handle, dq.ptr, f64, 2, 30, 90, dc.ptr, 3, 0)
    try:
        # count only
        assert lib.xc_contour_segments_dev(*head, 0, dn.ptr, None, None, None) == 1
        assert np.array_equal(dn.download((2, 3), np.uint64), ref[0])
        # one record short: 1, and the record arrays are not touched
        sent = np.full(total * 6, -12345, dtype=np.int64)
        rec = ctx.to_device(sent)
        try:
            ptrs = (rec.ptr, rec.ptr + total * 8, rec.ptr + total * 16)
            ctx._check(lib.xc_memset(ctx.handle, dn.ptr, 0xff, 48))
            assert lib.xc_contour_segments_dev(*head, total - 1, dn.ptr, *ptrs) == 1
            assert np.array_equal(dn.download((2, 3), np.uint64), ref[0])
            assert np.array_equal(rec.download((total * 6,), np.int64), sent)
            # exactly enough: XC_OK and the records
            assert lib.xc_contour_segments_dev(*head, total, dn.ptr, *ptrs) == nat.XC_OK
            ef, et = rec.download((total,), np.int64), rec.download((total,), np.int64, total * 8)
            pts = rec.download((total, 4), np.float64, total * 16)
        finally:
            rec.free()
        o = np.lexsort((ef, np.repeat(np.arange(6), ref[0].ravel().astype(np.int64))))
        same_records((ref[0], ef[o], et[o], pts[o]), ref, '_dev form')
        # capacity > 0 without record arrays is an error
        assert lib.xc_contour_segments_dev(*head, 5, dn.ptr, None, None, None) == nat.XC_EBADARG
    finally:
        for b in (dq, dc, dn):
            b.free()
    # the host form: the same protocol on host arrays
    cnt = np.zeros((2, 3), dtype=np.uint64)
    hhead = (ctx.handle, q.ctypes.data, f64, 2, 30, 90, lv.ctypes.data, 3, 0)
    assert lib.xc_contour_segments(*hhead, 0, cnt.ctypes.data, None, None, None) == 1
    assert np.array_equal(cnt, ref[0])
    ef, et, pts = np.full(total, -1, dtype=np.int64), np.full(total, -1, dtype=np.int64), np.full((total, 4), -1.0)
    assert lib.xc_contour_segments(*hhead, total - 1, cnt.ctypes.data, ef.ctypes.data, et.ctypes.data, pts.ctypes.data) == 1
    assert (ef == -1).all() and (et == -1).all() and (pts == -1.0).all()
    assert lib.xc_contour_segments(*hhead, total, cnt.ctypes.data, ef.ctypes.data, et.ctypes.data, pts.ctypes.data) == nat.XC_OK
    o = np.lexsort((ef, np.repeat(np.arange(6), cnt.ravel().astype(np.int64))))
    same_records((cnt, ef[o], et[o], pts[o]), ref, 'host form')
    # descending contours and NaN are refused
    bad = np.array([0.5, 0.0, 0.7])
    assert lib.xc_contour_segments(ctx.handle, q.ctypes.data, f64, 2, 30, 90, bad.ctypes.data, 3, 0, 0, cnt.ctypes.data, None, None, None) == nat.XC_EEDGES
    with pytest.raises(nat.XContourHipError):
        ctx.contour_segments(q, np.array([0.0, np.nan]))


def test_two_calls_give_the_same_records(ctx):
    q = field('saddle', (2, 70, 520), seed=12).astype(np.float32)
    lv = np.linspace(-1.5, 1.5, 11)
    a, b = ctx.contour_segments(q, lv), ctx.contour_segments(q, lv)
    same_records(a, b)


# K12 runs K10's tile walk and level search (xc_cell_walk.h, xc_levels.h): the edges K10 is pinned at (test_gpu_clen_variants.py)
EDGE_X = [1, 62, 63, 64, 251, 252, 253, 504, 505]
EDGE_Y = [1, 4, 5, 32, 33]


@pytest.mark.parametrize('ncy', EDGE_Y)
def test_tile_and_wave_edges(ctx, ncy):
    """nx - 1 across the wave (63 cells) and tile (252) boundaries, ny - 1 across the row batches (4) and tiles (32); two slabs,
    17 uneven levels, float32 and float64"""
    for ncx in EDGE_X:
        rng = np.random.default_rng(100 * ncy + ncx)
        lv = np.sort(rng.uniform(-2.0, 2.0, 17))
        for dt in (np.float32, np.float64):
            q = field('random', (2, ncy + 1, ncx + 1), seed=ncx * ncy + 1).astype(dt)
            got = check(ctx, q, lv, 'cells %dx%d %s' % (ncy, ncx, np.dtype(dt).name))
            assert got[0].sum() > 0


def on_and_next_to(q, lv, rng, dt):
    """corners exactly on a level and one ulp (of the tracer dtype) to either side"""
    S, ny, nx = q.shape
    for s in range(S):
        j, i = rng.integers(0, ny, 300), rng.integers(0, nx, 300)
        v = dt(lv[rng.integers(0, lv.size, 300)])
        q[s, j, i] = np.where(np.arange(300) % 3 == 0, v, np.where(np.arange(300) % 3 == 1, np.nextafter(v, dt(np.inf)),
                                                                     np.nextafter(v, dt(-np.inf))))
    return q


@pytest.mark.parametrize('dt', [np.float32, np.float64])
@pytest.mark.parametrize('kind', ['f32-linspace-300', 'f32-linspace-1e-4'])
def test_equally_spaced_search_edges(ctx, kind, dt):
    """equally spaced levels rounded through float32 (the arithmetic search and its verifying read), corners on levels and one ulp off"""
    rng = np.random.default_rng(len(kind))
    shape = (2, 53, 97)
    if kind == 'f32-linspace-300':
        lv = np.linspace(299.0, 301.0, 41).astype(np.float32).astype(np.float64)
        base = 300.0 + 0.8 * field('random', shape, seed=1)
    else:
        lv = np.linspace(-1e-4, 1e-4, 33).astype(np.float32).astype(np.float64)
        base = 0.7e-4 * field('random', shape, seed=3)
    q = on_and_next_to(base.astype(dt), lv, rng, dt)
    got = check(ctx, q, lv, kind)
    assert (got[0] > 0).all()


# ------------------------------------------------------------------ one call, batches of 2 + 1 slabs, a resident tracer
def batching_case(dt):
    """the smallest stack with more than one batch and an unequal last one, a seam column, and an empty range beside a full one:
    (3, 9, 12), five levels per slab of which the last lies above the field, the last slab -- a batch of its own -- all NaN"""
    q = field('random', (3, 9, 12), seed=31).astype(dt)
    q[2] = np.nan
    lv = np.array([-0.8, -0.3, 0.1, 0.6, 50.0])[None, :] + 0.07 * np.arange(3)[:, None]
    return q, lv


def three_ways(ctx, q, call):
    """call() (a) as it is, (b) in batches of 2 + 1 slabs, (c) on the device mirror of `q`"""
    a = call()
    cap = ctx.max_batch_bytes
    try:
        ctx.max_batch_bytes = 2 * q[0].nbytes + 8
        assert ctx._batches(3, q[0].nbytes) == [(0, 2), (2, 3)]
        b = call()
    finally:
        ctx.max_batch_bytes = cap
    try:
        ctx.keep_resident(q)
        assert ctx.resident_ptr(q)
        c = call()
    finally:
        ctx.release_resident(q)
    return a, b, c


@pytest.mark.parametrize('periodic', [False, True])
@pytest.mark.parametrize('dt', [np.float32, np.float64])
def test_batches_and_a_resident_tracer_give_the_same_records(ctx, dt, periodic):
    q, lv = batching_case(dt)
    a, b, c = three_ways(ctx, q, lambda: ctx.contour_segments(q, lv, periodic=periodic))
    cnt = a[0].astype(np.int64)
    assert (cnt[:2, :4] > 0).all() and (cnt[:2, 4] == 0).all() and (cnt[2] == 0).all()
    same_records(b, a, 'batches of 2 + 1')
    same_records(c, a, 'resident')
    for r in (b, c):
        assert [v.dtype for v in r] == [v.dtype for v in a] and type(r) is tuple
