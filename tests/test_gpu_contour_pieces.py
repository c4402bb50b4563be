"""Contour2D.cal_contour_pieces / Context.contour_pieces / xc_contour_pieces_dev (K13) on the GPU against the restatement
contour_pieces_ref: the integer fields and the row extents equal, `length` within 1e-12 * length (K10's own bar), `area` on a
Cartesian plane BIT FOR BIT the restatement's math.fsum (its terms are the kernel's: test_cpiece_records_host.py shows that the
restatement's np.interp coordinates are the separately rounded ones), on the sphere within 1e-12 * fsum(|terms|) (the sum is signed
and cancels; the device sin is not the host's); every facade call is made twice and compared bit for bit."""
import math

import numpy as np
import pytest

import clength_ref as CR
import contour_pieces_ref as PR
import xcontour_amd as xa
from xcontour_amd import _native as nat

pytestmark = pytest.mark.gpu

FIELDS = ('first_edge', 'nseg', 'closed', 'winding', 'length', 'area', 'y_min', 'y_max')


def facade(q, y, x, lead=()):
    dims = tuple('d%d' % i for i in range(len(lead))) + ('latitude', 'longitude')
    c = {'latitude': y, 'longitude': x}
    c.update({'d%d' % i: np.arange(n) for i, n in enumerate(lead)})
    tr = xa.DataArray(q, dims, c, 'q')
    return xa.Contour2D(tr, np.ones(len(y)), {'X': 'longitude', 'Y': 'latitude'}, {'Y': 'latitude'}, dtype=np.float64)


def same_table(a, b, what=''):
    """two structured arrays, every field bit for bit"""
    assert a.dtype == b.dtype and a.shape == b.shape, what
    for f in a.dtype.names:
        va, vb = a[f], b[f]
        if va.dtype.kind == 'f':
            va, vb = va.view(np.int64), vb.view(np.int64)
        assert np.array_equal(va, vb), '%s: field %s differs between two calls' % (what, f)


def twice(cm, lv, **kw):
    """the facade call, made twice: the same bits"""
    a, b = cm.cal_contour_pieces(lv, **kw), cm.cal_contour_pieces(lv, **kw)
    flat = lambda o: [t for s in o for t in s] if isinstance(o[0], list) else o
    for k, (ta, tb) in enumerate(zip(flat(a), flat(b))):
        same_table(ta, tb, 'level %d' % k)
    return a


def ref_period(periodic, latlon):
    """the period the facade hands to the library (Contour2D._x_period)"""
    if periodic is None or periodic is False:
        return None
    P = 360.0 if periodic is True else float(periodic)
    return float(np.float64(np.deg2rad(np.float32(P)))) if latlon else P


def check_level(got, ref, y, what='', latlon=False):
    """one level: the facade's table against the restatement's"""
    assert got.dtype.names == FIELDS, what
    assert got.size == ref.size, '%s: %d pieces, restatement %d' % (what, got.size, ref.size)
    for f in ('first_edge', 'nseg', 'closed', 'winding'):
        assert np.array_equal(got[f], ref[f]), '%s: %s' % (what, f)
    if not got.size:
        return
    yg = np.asarray(y, dtype=np.float64)
    ya, yb = np.interp(ref['row_min'], np.arange(yg.size), yg), np.interp(ref['row_max'], np.arange(yg.size), yg)
    assert np.array_equal(got['y_min'], np.minimum(ya, yb)) and np.array_equal(got['y_max'], np.maximum(ya, yb)), what + ': extent'
    dl = np.abs(got['length'] - ref['length'])
    assert (dl <= 1e-12 * ref['length']).all(), '%s: length off by %g relative' % (what, float(np.max(dl / np.maximum(ref['length'], 1e-300))))
    cl = ref['closed']
    assert np.isnan(got['area'][~cl]).all() and not np.isnan(got['area'][cl]).any(), what + ': area is NaN exactly for open pieces'
    da = np.abs(got['area'][cl] - ref['area'][cl])
    if not latlon:                                                           # every term is the restatement's: the exact sum, rounded once
        bad = np.flatnonzero(got['area'][cl].view(np.int64) != ref['area'][cl].view(np.int64))
        assert bad.size == 0, '%s: area of %d rings is not fsum of its terms, first %r != %r' % (
            what, bad.size, float(got['area'][cl][bad[0]]), float(ref['area'][cl][bad[0]]))
    assert (da <= 1e-12 * ref['area_abs'][cl]).all(), '%s: area off by %g of fsum(|terms|)' % (what, float(np.max(da / np.maximum(ref['area_abs'][cl], 1e-300))))


def check_plane(got, q2d, lv, y, x, latlon=False, periodic=False, what=''):
    fy, fx = CR.plane_coords(y, x, latlon)
    ref = PR.pieces(np.asarray(q2d, dtype=np.float64), lv, fy, fx, latlon, ref_period(periodic, latlon))
    assert len(got) == len(ref)
    for k in range(len(ref)):
        check_level(got[k], ref[k], y, '%s level %d' % (what, k), latlon)
    return ref


# ------------------------------------------------------------------ noise with NaN cells
NY, NX = 97, 301


@pytest.fixture(scope='module')
def noise():
    rng = np.random.default_rng(23)
    q = rng.standard_normal((NY, NX))
    q[rng.random(q.shape) < 0.03] = np.nan
    y, x = np.arange(NY) * 1.5 - 72.0, np.arange(NX) * 1.125                 # exact in float32, |lat| < 90, one lap short of 360
    lv = np.concatenate([[-9.0], np.linspace(-2.0, 2.0, 8), [np.nan, 11.0]])
    assert lv.size == 11
    return q, y, x, lv


@pytest.fixture(scope='module')
def noise_default(noise):
    """the Cartesian tables under the default workspace cap, computed once"""
    q, y, x, lv = noise
    return twice(facade(q, y, x), lv)


@pytest.mark.parametrize('latlon', [False, True])
def test_noise_with_nan_cells(noise, noise_default, latlon):
    q, y, x, lv = noise
    cm = facade(q, y, x)
    got = twice(cm, lv, latlon=True) if latlon else noise_default
    ref = check_plane(got, q, lv, y, x, latlon, what='latlon=%s' % latlon)
    assert got[0].size == 0 and got[-2].size == 0 and got[-1].size == 0      # out of range, NaN, out of range
    n = np.concatenate([r['nseg'] for r in ref])
    cl = np.concatenate([r['closed'] for r in ref])
    assert n.size > 2000 and (n[cl] <= 8).sum() > 500 and (~cl).sum() > 100   # many few-segment rings, open pieces beside NaN cells
    # the lengths of a level's pieces add up to cal_contour_lengths
    tot = cm.cal_contour_lengths(lv, latlon=latlon).values
    for k in range(lv.size):
        if np.isnan(tot[k]):
            assert got[k].size == 0 or got[k]['length'].sum() == 0.0
        else:
            assert abs(math.fsum(got[k]['length']) - tot[k]) <= 1e-12 * tot[k], k


def test_piece_order_and_flags_are_those_of_find_contours(noise, noise_default):
    """the pieces of a level come in find_contours' order (by the smallest grid-edge id), with its closed flags and its count;
    polyline by polyline the lengths agree (the coordinates are exact in float32, so both see the same plane)"""
    q, y, x, lv = noise
    polys, closed = facade(q, y, x).find_contours(lv, return_closed=True)
    for k in range(lv.size):
        t = noise_default[k]
        assert t.size == len(polys[k]) and t['closed'].tolist() == list(closed[k]), k
        assert (np.diff(t['first_edge']) > 0).all()
        pl = np.array([xa.polyline_length(p) for p in polys[k]])
        assert np.allclose(t['length'], pl, rtol=1e-9, atol=0)


def test_a_piece_of_coincident_points_is_kept_with_length_zero():
    """find_contours drops a polyline left with fewer than two distinct vertices; cal_contour_pieces does NOT mirror that: the
    piece stays, with length 0.  A node AT the level among nodes above it: its four cells emit one segment each, all four with
    both end points on the node -- one ring of four segments and of length 0."""
    q = np.ones((9, 11))
    q[4, 5] = 0.0
    y, x = np.arange(9) * 1.0, np.arange(11) * 2.0
    cm = facade(q, y, x)
    (t,) = twice(cm, np.array([0.0]))
    assert cm.find_contours(np.array([0.0])) == [[]]
    assert t.size == 1 and int(t['nseg'][0]) == 4 and bool(t['closed'][0]) and t['length'][0] == 0.0 and t['area'][0] == 0.0
    assert t['y_min'][0] == 4.0 and t['y_max'][0] == 4.0
    check_plane([t], q, [0.0], y, x)


# ------------------------------------------------------------------ the round count on either side of a power of two
@pytest.mark.parametrize('nx', [127, 128, 129])
def test_row_field_periodic_and_plain(nx):
    ny = 5
    q = np.repeat(np.arange(ny, dtype=np.float64)[:, None], nx, axis=1) + 0.25
    y, x = np.arange(ny) * 2.0 + 1.0, np.arange(nx) * 0.5
    cm = facade(q, y, x)
    lv = np.array([2.0])
    (t,) = twice(cm, lv, periodic=nx * 0.5)
    check_plane([t], q, lv, y, x, periodic=nx * 0.5, what='ring')
    assert t.size == 1 and int(t['nseg'][0]) == nx and bool(t['closed'][0]) and abs(int(t['winding'][0])) == 1
    y0 = 1.0 + 2.0 * 1.75
    assert abs(t['length'][0] - nx * 0.5) <= 1e-12 * nx and abs(abs(t['area'][0]) - y0 * nx * 0.5) <= 1e-12 * y0 * nx
    (t,) = twice(cm, lv)
    check_plane([t], q, lv, y, x, what='plain')
    assert t.size == 1 and int(t['nseg'][0]) == nx - 1 and not t['closed'][0] and np.isnan(t['area'][0]) and t['winding'][0] == 0


# ------------------------------------------------------------------ one long ring
def test_spiral_ring_float64_and_float32():
    n = 64
    yy, xx = np.meshgrid(np.arange(n) - 31.5 + 0.13, np.arange(n) - 31.5 - 0.21, indexing='ij')
    r, th = np.hypot(yy, xx), np.arctan2(yy, xx)
    q = np.minimum(np.cos(2.0 * np.pi * r / 3.0 - th), np.minimum((31.0 - r) / 2.0, (r - 1.5) / 2.0))
    y, x = np.arange(n) * 1.0, np.arange(n) * 0.5
    for qq in (q, q.astype(np.float32)):
        (t,) = twice(facade(qq, y, x), np.array([0.0]))
        check_plane([t], qq, [0.0], y, x, what=str(qq.dtype))
        big = int(np.argmax(t['nseg']))
        assert int(t['nseg'][big]) > 2000 and bool(t['closed'][big])       # one ring through every block of the launch


# ------------------------------------------------------------------ leading dims, per-slab and unsorted levels
def test_leading_dims_per_slab_and_unsorted_levels():
    rng = np.random.default_rng(22)
    q = rng.standard_normal((2, 3, 25, 40)).astype(np.float32)
    y, x = np.linspace(0.0, 48.0, 25), np.linspace(0.0, 78.0, 40)
    cm = facade(q, y, x, lead=(2, 3))
    lv = np.array([0.5, -1.0, np.nan, 1.5, 0.0, 9.0])
    got = twice(cm, lv)
    assert len(got) == 6 and all(len(g) == 6 for g in got)
    for s in range(6):
        check_plane(got[s], q.reshape(6, 25, 40)[s], lv, y, x, what='slab %d' % s)
        assert got[s][2].size == 0 and got[s][5].size == 0 and got[s][0].size > 0
    per = rng.uniform(-1.0, 1.0, (2, 3, 4))                                  # per slab, in no order
    ctr = xa.DataArray(per, ('d0', 'd1', 'contour'), {'d0': np.arange(2), 'd1': np.arange(3), 'contour': np.arange(4.0)}, 'q')
    got = twice(cm, ctr)
    for s in range(6):
        check_plane(got[s], q.reshape(6, 25, 40)[s], per.reshape(6, 4)[s], y, x, what='per-slab levels, slab %d' % s)


# ------------------------------------------------------------------ the barotropic field on the sphere, periodic
def test_barotropic_field_periodic_latlon(baro):
    q, lat, lon = baro
    cm = facade(q, lat, lon)
    lv = np.linspace(float(q.min()), float(q.max()), 21)
    got = twice(cm, lv, latlon=True, periodic=True)
    check_plane(got, q, lv, lat, lon, latlon=True, periodic=True, what='baro')
    assert any((t['closed'] & (t['winding'] != 0)).any() for t in got)       # a ring round the pole
    tot = cm.cal_contour_lengths(lv, latlon=True, periodic=True).values
    for k in range(lv.size):
        if np.isnan(tot[k]):
            assert got[k].size == 0, k
        else:
            assert got[k].size > 0 and abs(math.fsum(got[k]['length']) - tot[k]) <= 1e-12 * tot[k], k


# ------------------------------------------------------------------ the workspace cap: many groups, the same bits
def test_workspace_cap_does_not_change_the_result(noise, noise_default):
    q, y, x, lv = noise
    cm = facade(q, y, x)
    try:
        for cap in (1, 3 * 2 * NY * NX * 4):                                 # one range per group; three ranges per group
            cm.ctx.set_cpiece_workspace(cap)
            got = cm.cal_contour_pieces(lv)
            for k in range(lv.size):
                same_table(got[k], noise_default[k], 'cap %d, level %d' % (cap, k))
    finally:
        cm.ctx.set_cpiece_workspace(1 << 30)


# ------------------------------------------------------------------ the C entry: rows, the capacity protocol
def test_c_entry_rows_and_capacity_one_short(noise):
    q, y, x, lv = noise
    ctx = nat.default_context(0)
    lvs = np.sort(np.where(np.isnan(lv), np.inf, lv))
    N = lvs.size
    fy, fx = CR.plane_coords(y, x, False)
    pc, tab = ctx.contour_pieces(q[None], lvs, fy, fx)
    ref = PR.pieces(q, lvs, fy, fx)
    assert np.array_equal(pc.ravel().astype(np.int64), [r.size for r in ref])
    allref = np.concatenate(ref)
    for f in ('first_edge', 'nseg', 'closed', 'winding', 'row_min', 'row_max'):
        assert np.array_equal(tab[f], allref[f]), f
    npiece = int(pc.sum())
    # the C entry with a capacity one short of the total: 1, piece_count written, the record arrays untouched
    lib = ctx.lib
    with ctx._temporaries([np.ascontiguousarray(q), lvs, fy, fx], [N * 8, N * 8]) as (dq, dc, dy, dx, dn, dpc):
        head = (ctx.handle, dq.ptr, nat.XC_F64, 1, NY, NX, dc.ptr, N, 0)
        assert lib.xc_contour_segments_dev(*head, 0, dn.ptr, None, None, None) in (0, 1)
        total = int(dn.download((N,), np.uint64).sum())
        fill = np.full(npiece, 0x5a5a5a5a5a5a5a5a, dtype=np.uint64)
        with ctx._temporaries([fill] * 8 + [np.full(N, 77, dtype=np.uint64)], [total * 8, total * 8, total * 32]) as bufs:
            rec, dpc2, (df, dt, dp) = bufs[:8], bufs[8], bufs[9:]
            assert lib.xc_contour_segments_dev(*head, total, dn.ptr, df.ptr, dt.ptr, dp.ptr) == 0
            args = (ctx.handle, N, dn.ptr, df.ptr, dt.ptr, dp.ptr, NY, NX, 0, dy.ptr, dx.ptr, 0.0, 0.0)
            rc = lib.xc_contour_pieces_dev(*args, npiece - 1, dpc2.ptr, *[b.ptr for b in rec])
            assert rc == 1
            assert np.array_equal(dpc2.download((N,), np.uint64), pc.ravel())
            for b in rec:
                assert np.array_equal(b.download((npiece,), np.uint64), fill)
            # and with room for all of them: written
            assert lib.xc_contour_pieces_dev(*args, npiece, dpc2.ptr, *[b.ptr for b in rec]) == 0
            fe = rec[0].download((npiece,), np.int64)
            o = np.lexsort((fe, np.repeat(np.arange(N), pc.ravel().astype(np.int64))))
            assert np.array_equal(fe[o], tab['first_edge'])
            assert np.array_equal(rec[4].download((npiece,), np.float64)[o].view(np.int64), tab['length'].view(np.int64))


# ------------------------------------------------------------------ one call, batches of 2 + 1 slabs, a resident tracer
def batching_case(dt):
    """as in test_gpu_contour_segments.py: (3, 9, 12), five levels per slab with the last above the field, the last slab all NaN"""
    q = np.random.default_rng(31).standard_normal((3, 9, 12)).astype(dt)
    q[2] = np.nan
    lv = np.array([-0.8, -0.3, 0.1, 0.6, 50.0])[None, :] + 0.07 * np.arange(3)[:, None]
    return q, lv


def in_batches_of_two(ctx, q, call):
    cap = ctx.max_batch_bytes
    try:
        ctx.max_batch_bytes = 2 * q[0].nbytes + 8
        assert ctx._batches(3, q[0].nbytes) == [(0, 2), (2, 3)]
        return call()
    finally:
        ctx.max_batch_bytes = cap


@pytest.mark.parametrize('period', [None, 24.0])
@pytest.mark.parametrize('dt', [np.float32, np.float64])
def test_batches_and_a_resident_tracer_give_the_same_table(dt, period):
    ctx = nat.default_context(0)
    q, lv = batching_case(dt)
    y, x = np.arange(9) * 1.5, np.arange(12) * 2.0
    call = lambda: ctx.contour_pieces(q, lv, y, x, period=period)
    a = call()
    b = in_batches_of_two(ctx, q, call)
    try:
        ctx.keep_resident(q)
        assert ctx.resident_ptr(q)
        c = call()
    finally:
        ctx.release_resident(q)
    pc = a[0].astype(np.int64)
    assert (pc[:2, :4] > 0).all() and (pc[:2, 4] == 0).all() and (pc[2] == 0).all() and a[1].size == pc.sum()
    for r, what in ((b, 'batches of 2 + 1'), (c, 'resident')):
        assert type(r) is tuple and r[0].dtype == np.uint64 and np.array_equal(r[0], a[0]), what
        same_table(r[1], a[1], what)


@pytest.mark.parametrize('periodic', [False, True])
@pytest.mark.parametrize('dt', [np.float32, np.float64])
def test_facade_in_batches_with_descending_levels(dt, periodic):
    """find_contours and cal_contour_pieces on a (time, lat, lon) tracer, levels descending: one call against batches of 2 + 1"""
    q, _ = batching_case(dt)
    lat, lon = -60.0 + 15.0 * np.arange(9), 30.0 * np.arange(12)
    cm = facade(q, lat, lon, lead=(3,))
    lv = np.array([50.0, 0.6, 0.1, -0.3, -0.8])
    fc = lambda: cm.find_contours(lv, return_closed=True, return_winding=True, periodic=periodic)
    pcs = lambda: cm.cal_contour_pieces(lv, latlon=periodic, periodic=periodic)
    (pa, ca, wa), ta = fc(), pcs()
    (pb, cb, wb), tb = in_batches_of_two(cm.ctx, q, fc), in_batches_of_two(cm.ctx, q, pcs)
    assert ca == cb and wa == wb
    for s in range(3):
        assert len(pa[s]) == len(pb[s]) == len(ta[s]) == len(tb[s]) == 5
        for k in range(5):
            assert len(pa[s][k]) == len(pb[s][k])
            for u, v in zip(pa[s][k], pb[s][k]):
                assert u.shape == v.shape and np.array_equal(np.ascontiguousarray(u).view(np.int64), np.ascontiguousarray(v).view(np.int64))
            same_table(ta[s][k], tb[s][k], 'slab %d level %d' % (s, k))
            assert (ta[s][k].size > 0) == (s < 2 and k > 0) and (len(pa[s][k]) > 0) == (s < 2 and k > 0)
