"""Context.contour_overturning / Contour2D.cal_contour_overturning (K16) on the GPU against the restatement coverturn_ref applied to
Context.contour_segments of the same input: integers equal, rows bit for bit, NaN in the same places -- no tolerance anywhere.
Beside it an identity that knows nothing of segments: on a NaN-free plane, with levels that equal no node value, 'all' counts in
column c the rows r where q[r, c] and q[r + 1, c] lie on different sides of the level."""
import numpy as np
import pytest

import coverturn_ref as OR
import xcontour_amd as xa
from xcontour_amd import _native as nat

pytestmark = pytest.mark.gpu

OPTIONS = [(False, 'all'), (True, 'all'), (True, 'circumpolar'), (True, 'main')]
IDS = ['plain all', 'ring all', 'ring circumpolar', 'ring main']


def restated(ctx, q, lv, periodic, select):
    """the restatement on the records Context.contour_segments gives for the same input -> the seven arrays, shaped like the call's"""
    cnt, ef, et, pts = ctx.contour_segments(q, lv, periodic=periodic)
    nslab, ny, nx = q.shape
    ref = OR.overturning(cnt.ravel(), ef, et, pts, ny, nx, 1 if periodic else 0, select)
    return [ref[f].reshape(cnt.shape + ref[f].shape[1:]) for f in OR.FIELDS], cnt


def same(got, ref, what=''):
    assert isinstance(got, tuple) and len(got) == 7, what
    bad = OR.differences(dict(zip(OR.FIELDS, got)), dict(zip(OR.FIELDS, ref)))
    assert bad == [], '%s: %r differ' % (what, bad)


def noise_plane(dt):
    """40 x 67 noise with blocks of NaN; the first and the last level lie outside the field: empty ranges at both ends"""
    rng = np.random.default_rng(41)
    q = rng.standard_normal((2, 40, 67))
    q[0, 5:9, 20:31] = np.nan
    q[1, 30:33, 0:4] = np.nan
    q[1, 12, 66] = np.nan
    return q.astype(dt), np.concatenate([[-9.0], np.linspace(-1.5, 1.5, 5), [11.0]])


@pytest.mark.parametrize('periodic,select', OPTIONS, ids=IDS)
@pytest.mark.parametrize('dt', [np.float32, np.float64])
def test_noise_with_nan_blocks_and_per_slab_levels(ctx, dt, periodic, select):
    q, lv = noise_plane(dt)
    for levels in (lv, np.stack([lv, lv + 0.125])):
        got = ctx.contour_overturning(q, levels, periodic=periodic, select=select)
        ref, cnt = restated(ctx, q, levels, periodic, select)
        same(got, ref, 'noise')
        same(ctx.contour_overturning(q, levels, periodic=periodic, select=select), got, 'the second call')
        assert (cnt[:, 0] == 0).all() and (cnt[:, -1] == 0).all() and (cnt[:, 1:-1] > 100).all()
        assert not got[0][:, 0].any() and np.isnan(got[1][:, -1]).all() and (got[4][:, 0] == -1).all()
        assert [a.shape for a in got] == [(2, 7, 67)] * 3 + [(2, 7)] * 4
        assert [a.dtype for a in got] == [np.int32, np.float64, np.float64, np.int32, np.int64, np.int64, np.int32]
    if select == 'all':
        assert got[0].sum() > 1000 and got[3].max() > 20


@pytest.mark.parametrize('periodic,select', OPTIONS, ids=IDS)
def test_the_2_x_3_plane(ctx, periodic, select):
    q = np.array([[[0.0, 1.0, 0.0], [1.0, 0.0, 1.0]], [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]], [[2.0, 2.0, 2.0], [2.0, 2.0, 2.0]]])
    lv = np.array([0.25, 0.5, 3.0])
    got = ctx.contour_overturning(q, lv, periodic=periodic, select=select)
    same(got, restated(ctx, q, lv, periodic, select)[0], '2 x 3')
    assert got[0][1].tolist() == [[1, 1, 1], [1, 1, 1], [0, 0, 0]] and not got[0][2].any()          # a zonal step; a flat slab
    assert (got[1][1, 0] == 0.25).all() and (got[2][1, 1] == 0.5).all()
    if periodic:
        assert got[5][1].tolist() == [3, 3, 0] and np.abs(got[6][1]).tolist() == [1, 1, 0]


@pytest.mark.parametrize('periodic,select', OPTIONS, ids=IDS)
def test_the_barotropic_field_at_21_levels(ctx, baro, periodic, select):
    q = np.asarray(baro[0], dtype=np.float64)[None]
    lv = np.linspace(float(q.min()), float(q.max()), 21)
    got = ctx.contour_overturning(q, lv, periodic=periodic, select=select)
    ref, cnt = restated(ctx, q, lv, periodic, select)
    same(got, ref, 'baro')
    if periodic:
        assert (got[4][0] >= 0).sum() >= 10                                  # most levels have a ring round the pole ...
        if select == 'main':
            assert (got[0][0][got[4][0] >= 0] >= 1).all() and (got[0] >= 3).any()   # ... which meets every meridian, some of them thrice


def batching_case(dt):
    rng = np.random.default_rng(42)
    q = rng.standard_normal((3, 9, 12)).astype(dt)
    q[:, 4:] += 3.0                                                          # a step the middle levels follow round the ring
    q[2, 0, 0] = np.nan
    lv = np.array([-0.8, 0.1, 1.5, 2.1, 50.0])[None, :] + 0.07 * np.arange(3)[:, None]
    return q, lv


@pytest.mark.parametrize('periodic,select', [(False, 'all'), (True, 'main')], ids=['plain all', 'ring main'])
@pytest.mark.parametrize('dt', [np.float32, np.float64])
def test_unequal_batches_and_a_resident_tracer_give_the_same_bits(dt, periodic, select):
    ctx = nat.default_context(0)
    q, lv = batching_case(dt)
    call = lambda: ctx.contour_overturning(q, lv, periodic=periodic, select=select)
    a = call()
    per = q[0].nbytes + lv.shape[1] * q.shape[2] * 20                        # what a slab stages: its plane and 20 bytes per (contour, column)
    cap = ctx.max_batch_bytes
    try:
        ctx.max_batch_bytes = 2 * per + 8
        assert ctx._batches(3, per) == [(0, 2), (2, 3)]
        b = call()
        ctx.max_batch_bytes = 2 * q[0].nbytes + 8                            # room for two planes, not for two slabs' outputs
        assert ctx._batches(3, per) == [(0, 1), (1, 2), (2, 3)]
        b1 = call()
    finally:
        ctx.max_batch_bytes = cap
    try:
        ctx.keep_resident(q)
        assert ctx.resident_ptr(q)
        c = call()
    finally:
        ctx.release_resident(q)
    for r, what in ((b, 'batches of 2 + 1'), (b1, 'batches of 1'), (c, 'resident')):
        same(r, a, what)
    same(a, restated(ctx, q, lv, periodic, select)[0], 'batching case')
    assert a[0].any() and (a[3][:, 4] == 0).all()
    # a batch without segments is filled on the host: zeros, NaN and -1
    e = ctx.contour_overturning(q, lv + 100.0, periodic=periodic, select=select)
    assert not e[0].any() and np.isnan(e[1]).all() and np.isnan(e[2]).all() and not e[3].any() and (e[4] == -1).all() and not e[5].any() and not e[6].any()
    assert [x.shape for x in e] == [x.shape for x in a] and [x.dtype for x in e] == [x.dtype for x in a]


@pytest.mark.parametrize('periodic', [False, True])
def test_all_counts_the_sign_changes_down_every_column(ctx, periodic):
    """independent of every segment rule: a contour crosses the vertical edge between (r, c) and (r + 1, c) exactly when the two
    nodes lie on different sides of the level.  On the ring column 0 is not doubled by the seam cell."""
    rng = np.random.default_rng(43)
    q = rng.standard_normal((2, 33, 65))
    lv = np.array([-1.0, -0.3, 0.0, 0.45, 1.2])
    assert not np.isin(lv, q).any()
    got = ctx.contour_overturning(q, lv, periodic=periodic, select='all')
    above = q[:, None] > lv[None, :, None, None]                             # (slab, level, row, column)
    flips = above[:, :, 1:] != above[:, :, :-1]
    assert np.array_equal(got[0], flips.sum(axis=2).astype(np.int32))
    assert got[0].max() >= 3
    # the rows: the first and the last flip of the column, interpolated by K12 between the two node rows
    first = np.where(flips.any(axis=2), flips.argmax(axis=2), -1)
    has = first >= 0
    assert (np.floor(got[1][has]) == first[has]).all() and np.isnan(got[1][~has]).all()


def facade(q, y, x, lead=()):
    dims = tuple('d%d' % i for i in range(len(lead))) + ('latitude', 'longitude')
    c = {'latitude': y, 'longitude': x}
    c.update({'d%d' % i: np.arange(n) for i, n in enumerate(lead)})
    return xa.Contour2D(xa.DataArray(q, dims, c, 'q'), np.ones(len(y)), {'X': 'longitude', 'Y': 'latitude'}, {'Y': 'latitude'}, dtype=np.float64)


@pytest.mark.parametrize('descending', [False, True], ids=['latitude ascending', 'latitude descending'])
def test_facade_in_caller_order_with_coordinates_and_the_main_ring_among_the_pieces(descending):
    ctx = nat.default_context(0)
    q, _ = batching_case(np.float64)
    y, x = np.arange(9) * 1.5 - 6.0, np.arange(12) * 30.0
    if descending:
        y = y[::-1].copy()
    lv = np.array([2.1, -0.8, 1.5, np.nan, 0.1])                             # the caller's order; a NaN level has nothing
    cm = facade(q, y, x, lead=(3,))
    ds = cm.cal_contour_overturning(lv, periodic=True)
    assert list(ds) == ['ncross', 'y_lo', 'y_hi', 'nsel', 'main_first_edge', 'main_nseg', 'main_winding']
    assert ds['ncross'].dims == ('d0', 'contour', 'longitude') and ds['nsel'].dims == ('d0', 'contour')
    assert ds['ncross'].values.shape == (3, 5, 12) and np.array_equal(ds['y_lo'].coords['longitude'], x)
    order = np.argsort(np.where(np.isnan(lv), np.inf, lv), kind='stable')
    raw = ctx.contour_overturning(q, np.where(np.isnan(lv), np.inf, lv)[order], periodic=True, select='main')
    for name, v in zip(OR.FIELDS, raw):
        if name not in ('row_lo', 'row_hi'):
            assert np.array_equal(ds[name].values[:, order], v), name
    ya, yb = np.interp(raw[1], np.arange(9), y), np.interp(raw[2], np.arange(9), y)
    assert OR.same_bits(ds['y_lo'].values[:, order], np.minimum(ya, yb)) and OR.same_bits(ds['y_hi'].values[:, order], np.maximum(ya, yb))
    assert not ds['ncross'].values[:, 3].any() and (ds['main_first_edge'].values[:, 3] == -1).all()
    # the main ring under its key among cal_contour_pieces' records
    pieces = cm.cal_contour_pieces(lv, periodic=360.0)
    found = 0
    for s in range(3):
        for k in range(5):
            fe = int(ds['main_first_edge'].values[s, k])
            if fe < 0:
                assert not (pieces[s][k]['winding'] != 0).any()
                continue
            t = pieces[s][k][pieces[s][k]['first_edge'] == fe]
            assert t.size == 1 and t['closed'][0] and t['nseg'][0] == ds['main_nseg'].values[s, k] and t['winding'][0] == ds['main_winding'].values[s, k]
            assert (ds['ncross'].values[s, k] >= 1).all()                     # it goes round: it meets every meridian
            found += 1
    assert found >= 3
    # 'all' on the plain plane; the refusal names `periodic`
    plain = cm.cal_contour_overturning(lv, select='all')
    assert np.array_equal(plain['ncross'].values[:, order], ctx.contour_overturning(q, np.where(np.isnan(lv), np.inf, lv)[order], select='all')[0])
    with pytest.raises(Exception, match='periodic'):
        cm.cal_contour_overturning(lv)
    with pytest.raises(Exception, match='periodic'):
        ctx.contour_overturning(q, np.sort(lv[~np.isnan(lv)]), select='circumpolar')
    with pytest.raises(Exception, match='select'):
        cm.cal_contour_overturning(lv, periodic=True, select='largest')
