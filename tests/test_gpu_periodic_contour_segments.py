"""K12 with a periodic X direction (xc_contour_segments_periodic, Context.contour_segments(periodic=True)) on the GPU.  The
identity it is built on: the records are those of the plain call on the plane with column 0 appended as column nx, the edge ids
folded onto the ring and every range sorted again -- counts, e_from and e_to equal, pts bit for bit.  Both sides of the identity
are also held against the restatement (contour_join_periodic_ref / contour_join_ref)."""
import numpy as np
import pytest

import contour_join_periodic_ref as PJ
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


def no_id_repeats(rec, what=''):
    """inside a range no edge starts two segments and none ends two"""
    cnt, ef, et, _ = rec
    rng_of = np.repeat(np.arange(cnt.size), cnt.ravel().astype(np.int64))
    for e in (ef, et):
        pairs = np.stack([rng_of, e], axis=1)
        assert np.unique(pairs, axis=0).shape[0] == pairs.shape[0], what + ': an edge id repeats in a range'


def check(ctx, q, lv, what='', restate=True):
    nx = q.shape[-1]
    got = ctx.contour_segments(q, lv, periodic=True)
    assert got[0].dtype == np.uint64 and got[1].dtype == np.int64 and got[2].dtype == np.int64 and got[3].dtype == np.float64
    qe = PJ.extend(q)
    same_records(got, PJ.fold_records(ctx.contour_segments(qe, lv), nx), what + ' identity')
    if restate:
        same_records(got, PJ.stack_records(q.astype(np.float64), lv), what + ' restatement')
    no_id_repeats(got, what)
    if got[3].size:
        assert got[3][:, [1, 3]].min() >= 0.0 and got[3][:, [1, 3]].max() <= float(nx)
    return got


def field(kind, shape, seed=7):
    rng = np.random.default_rng(seed)
    if kind == 'saddle':
        return np.indices(shape[-2:]).sum(0) % 2 * 2.0 - 1.0 + 0.3 * rng.standard_normal(shape)       # checkerboard
    if kind == 'onlevel':
        return rng.integers(-2, 3, shape).astype(np.float64)                                            # nodes exactly on the levels
    q = rng.standard_normal(shape)
    if kind == 'nan':
        q[rng.random(shape) < 0.03] = np.nan
        q[..., 3:7, 0] = np.nan                                                                         # and on either side of the seam
        q[..., 11:13, -1] = np.nan
    return q


LEVELS = {'random': np.linspace(-2.0, 2.0, 13), 'saddle': np.linspace(-2.0, 2.0, 13), 'nan': np.linspace(-2.0, 2.0, 13),
          'onlevel': np.array([-2.0, -1.0, -0.5, 0.0, 1.0, 2.0])}


@pytest.mark.parametrize('kind', ['random', 'saddle', 'nan', 'onlevel'])
@pytest.mark.parametrize('dt', [np.float32, np.float64])
def test_identity_and_restatement(ctx, kind, dt):
    """2 slabs of 36 x 260: two tile rows and two tile columns, the last of each partial; shared and per-slab levels"""
    q = field(kind, (2, 36, 260)).astype(dt)
    lv = LEVELS[kind]
    got = check(ctx, q, lv, kind + ' shared')
    assert got[0].sum() > 2000
    # the seam cells emit: some segment lies in the cell column nx-1 .. nx
    assert (np.minimum(got[3][:, 1], got[3][:, 3]) >= 259.0).any() and (got[3][:, [1, 3]] == 260.0).any()
    check(ctx, q, lv[None, :] + 0.013 * np.arange(2)[:, None], kind + ' per slab')


@pytest.mark.parametrize('nx', [2, 63, 64, 65, 252, 253, 254, 505])
def test_the_seam_on_every_lane_role(ctx, nx):
    """the seam cell as lane 0, 61, 62, the first lane of the next wave, the last cell of a tile, the first of the next tile, and
    its right neighbour as a cell lane, the halo lane 63 and the first lane of a new tile; one tile row and two"""
    lv = np.array([-0.7, 0.0, 0.4])
    for ny in (2, 33, 34):
        for dt in (np.float32, np.float64):
            q = field('random', (2, ny, nx), seed=nx + ny).astype(dt)
            got = check(ctx, q, lv, '%d x %d %s' % (ny, nx, dt.__name__))
            assert got[0].sum() > 0


def test_one_column_is_refused_and_one_row_has_no_cells(ctx):
    lv = np.array([-0.7, 0.0, 0.4])
    with pytest.raises(nat.XContourHipError) as e:
        ctx.contour_segments(np.zeros((2, 9, 1)), lv, periodic=True)
    assert e.value.code == nat.XC_EBADARG
    q1 = field('random', (1, 9, 1))
    cnt = np.zeros((1, 3), dtype=np.uint64)
    dq, dc, dn = ctx.to_device(q1), ctx.to_device(lv), ctx.alloc(3 * 8)
    try:
        assert ctx.lib.xc_contour_segments_periodic_dev(ctx.handle, dq.ptr, nat.XC_F64, 1, 9, 1, dc.ptr, 3, 0, 0, dn.ptr, None, None,
                                                        None) == nat.XC_EBADARG
    finally:
        for b in (dq, dc, dn):
            b.free()
    assert ctx.lib.xc_contour_segments_periodic(ctx.handle, q1.ctypes.data, nat.XC_F64, 1, 9, 1, lv.ctypes.data, 3, 0, 0, cnt.ctypes.data,
                                                None, None, None) == nat.XC_EBADARG
    got = ctx.contour_segments(field('random', (2, 1, 9)), lv, periodic=True)
    assert got[0].shape == (2, 3) and got[0].sum() == 0 and got[1].size == 0 and got[3].shape == (0, 4)
    cnt[:] = 77
    q2 = field('random', (1, 1, 9))
    assert ctx.lib.xc_contour_segments_periodic(ctx.handle, q2.ctypes.data, nat.XC_F64, 1, 1, 9, lv.ctypes.data, 3, 0, 0, cnt.ctypes.data,
                                                None, None, None) == nat.XC_OK
    assert (cnt == 0).all()


def test_more_levels_than_one_group_and_a_single_level(ctx):
    q = field('random', (2, 9, 70), seed=9)
    N = nat.XC_CSEG_GROUP_LEVELS + 3
    check(ctx, q, np.sort(np.random.default_rng(1).uniform(-2.5, 2.5, N)), 'N = %d' % N)
    check(ctx, q, np.array([0.1]), 'N = 1')


def test_many_blocks_per_slab_and_many_slabs(ctx):
    lv = np.array([-1.0, -0.2, 0.0, 0.3, 1.1])
    big = field('nan', (1, 200, 1100), seed=2)            # 35 tiles, one block each; without the wrap 1099 cell columns
    one = check(ctx, big, lv, 'one large slab')
    check(ctx, field('random', (40, 20, 60), seed=4), lv, 'forty slabs')
    # the same plane alone and inside a stack: the same records
    stack = field('random', (5, 200, 1100), seed=6)
    stack[3] = big[0]
    got = ctx.contour_segments(stack, lv, periodic=True)
    off = np.concatenate([[0], np.cumsum(got[0].ravel().astype(np.int64))])
    a, b = off[3 * lv.size], off[4 * lv.size]
    same_records((got[0][3:4], got[1][a:b], got[2][a:b], got[3][a:b]), one, 'alone against inside a stack')


def test_capacity_protocol(ctx):
    q = field('random', (2, 30, 90), seed=8)
    lv = np.array([-0.5, 0.0, 0.5])
    ref = PJ.stack_records(q, lv)
    total = int(ref[0].sum())
    assert total > int(JR.stack_records(q, lv)[0].sum())
    lib, f64 = ctx.lib, nat.XC_F64
    dq, dc, dn = ctx.to_device(q), ctx.to_device(lv), ctx.alloc(2 * 3 * 8)
    head = (ctx.handle, dq.ptr, f64, 2, 30, 90, dc.ptr, 3, 0)
    try:
        # count only
        assert lib.xc_contour_segments_periodic_dev(*head, 0, dn.ptr, None, None, None) == 1
        assert np.array_equal(dn.download((2, 3), np.uint64), ref[0])
        # one record short: 1, and the record arrays are not touched
        sent = np.full(total * 6, -12345, dtype=np.int64)
        rec = ctx.to_device(sent)
        try:
            ptrs = (rec.ptr, rec.ptr + total * 8, rec.ptr + total * 16)
            ctx._check(lib.xc_memset(ctx.handle, dn.ptr, 0xff, 48))
            assert lib.xc_contour_segments_periodic_dev(*head, total - 1, dn.ptr, *ptrs) == 1
            assert np.array_equal(dn.download((2, 3), np.uint64), ref[0])
            assert np.array_equal(rec.download((total * 6,), np.int64), sent)
            # exactly enough: XC_OK and the records
            assert lib.xc_contour_segments_periodic_dev(*head, total, dn.ptr, *ptrs) == nat.XC_OK
            ef, et = rec.download((total,), np.int64), rec.download((total,), np.int64, total * 8)
            pts = rec.download((total, 4), np.float64, total * 16)
        finally:
            rec.free()
        o = np.lexsort((ef, np.repeat(np.arange(6), ref[0].ravel().astype(np.int64))))
        same_records((ref[0], ef[o], et[o], pts[o]), ref, '_dev form')
        assert lib.xc_contour_segments_periodic_dev(*head, 5, dn.ptr, None, None, None) == nat.XC_EBADARG
    finally:
        for b in (dq, dc, dn):
            b.free()
    # the host form: the same protocol on host arrays
    cnt = np.zeros((2, 3), dtype=np.uint64)
    hhead = (ctx.handle, q.ctypes.data, f64, 2, 30, 90, lv.ctypes.data, 3, 0)
    assert lib.xc_contour_segments_periodic(*hhead, 0, cnt.ctypes.data, None, None, None) == 1
    assert np.array_equal(cnt, ref[0])
    ef, et, pts = np.full(total, -1, dtype=np.int64), np.full(total, -1, dtype=np.int64), np.full((total, 4), -1.0)
    assert lib.xc_contour_segments_periodic(*hhead, total - 1, cnt.ctypes.data, ef.ctypes.data, et.ctypes.data, pts.ctypes.data) == 1
    assert (ef == -1).all() and (et == -1).all() and (pts == -1.0).all()
    assert lib.xc_contour_segments_periodic(*hhead, total, cnt.ctypes.data, ef.ctypes.data, et.ctypes.data, pts.ctypes.data) == nat.XC_OK
    o = np.lexsort((ef, np.repeat(np.arange(6), cnt.ravel().astype(np.int64))))
    same_records((cnt, ef[o], et[o], pts[o]), ref, 'host form')
    bad = np.array([0.5, 0.0, 0.7])
    assert lib.xc_contour_segments_periodic(ctx.handle, q.ctypes.data, f64, 2, 30, 90, bad.ctypes.data, 3, 0, 0, cnt.ctypes.data, None, None,
                                            None) == nat.XC_EEDGES


@pytest.mark.parametrize('dt', [np.float32, np.float64])
def test_plain_entry_points_are_what_they_were(ctx, dt):
    """the same inputs through the plain entry points, against the plain restatement: no seam cell, the plain ids"""
    for kind in ('random', 'saddle', 'nan', 'onlevel'):
        q = field(kind, (2, 36, 260)).astype(dt)
        same_records(ctx.contour_segments(q, LEVELS[kind]), JR.stack_records(q.astype(np.float64), LEVELS[kind]), kind)
        same_records(ctx.contour_segments(q, LEVELS[kind], periodic=False), JR.stack_records(q.astype(np.float64), LEVELS[kind]), kind)
    for nx in (2, 63, 64, 65, 252, 253, 254, 505):
        q = field('random', (2, 34, nx), seed=nx + 34).astype(dt)
        same_records(ctx.contour_segments(q, np.array([-0.7, 0.0, 0.4])), JR.stack_records(q.astype(np.float64), np.array([-0.7, 0.0, 0.4])),
                     'nx = %d' % nx)


def test_two_calls_give_the_same_records(ctx):
    q = field('saddle', (2, 70, 520), seed=12).astype(np.float32)
    lv = np.linspace(-1.5, 1.5, 11)
    a, b = ctx.contour_segments(q, lv, periodic=True), ctx.contour_segments(q, lv, periodic=True)
    same_records(a, b)
    no_id_repeats(a)
