"""The device join (K14) through Context.contour_polylines and trace_contours(join='device'), against the route it replaces:
Context.contour_segments, then the host join xc_join_segments.  Everything is compared bit for bit."""
import functools

import numpy as np
import pytest

import xcontour_amd as xa
from xcontour_amd import _native as nat

pytestmark = pytest.mark.gpu

DEFAULT_CAP = 1 << 30


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def noise_plane():
    """33 x 40 float64 noise with a NaN block: interior open ends, many few-cell rings; 7 levels, the first and the last two
    outside the field's range (empty ranges at the start and the end)"""
    rng = np.random.default_rng(41)
    q = rng.standard_normal((33, 40))
    q[12:17, 20:29] = np.nan
    lo, hi = float(np.nanmin(q)), float(np.nanmax(q))
    return q, np.array([lo - 1.0, -1.0, -0.25, 0.0, 0.6, hi + 0.5, hi + 1.0])


def reference(ctx, q, lv, periodic):
    """the parent route -> what Context.contour_polylines must return"""
    cnt, ef, et, pts = ctx.contour_segments(q, lv, periodic=periodic)
    off = np.concatenate([[0], np.cumsum(cnt.ravel().astype(np.int64))])
    walk, poff, closed, rpo = nat.join_segments(off, ef, et)
    return cnt, ef[walk], pts[walk], poff, closed, rpo


def same_result(got, ref, what=''):
    names = ('count', 'e_from_walk', 'pts_walk', 'poly_off', 'closed', 'rpo')
    assert len(got) == len(ref) == 6
    for name, g, r in zip(names, got, ref):
        assert g.dtype == r.dtype and g.shape == r.shape, '%s: %s is %s %s, expected %s %s' % (what, name, g.dtype, g.shape, r.dtype, r.shape)
        assert np.array_equal(bits(g), bits(r)) if r.dtype == np.float64 else np.array_equal(g, r), '%s: %s' % (what, name)


def cases(baro):
    q, lv = noise_plane()
    yield 'noise', q[None], lv, False
    yield 'noise, periodic', q[None], lv, True
    tiny = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 1.0]])
    yield '2 x 3', tiny[None], np.array([0.25, 0.5]), False
    yield '2 x 3, periodic', tiny[None], np.array([0.25, 0.5]), True
    b = np.asarray(baro[0], dtype=np.float64)
    bl = np.linspace(float(b.min()), float(b.max()), 9)[1:-1]
    yield 'baro', b[None], bl, False
    yield 'baro, periodic', b[None], bl, True


def test_records_in_walk_order_equal_the_host_join(ctx, baro):
    seen = {}
    for what, q, lv, periodic in cases(baro):
        got = ctx.contour_polylines(q, lv, periodic=periodic)
        ref = reference(ctx, q, lv, periodic)
        same_result(got, ref, what)
        seen[what] = got
    cnt, _, _, poff, closed, rpo = seen['noise']
    assert cnt[0, 0] == 0 and cnt[0, -1] == 0 and cnt[0, -2] == 0 and rpo[-1] > 30       # empty ranges at both ends
    assert closed.any() and not closed.all() and (np.diff(poff)[closed] <= 8).sum() > 10  # open ends and few-cell rings
    assert seen['2 x 3'][0].sum() > 0
    # the periodic barotropic plane: fewer open polylines than the plain one (rings that circle the pole are closed there)
    assert seen['baro, periodic'][4].sum() > seen['baro'][4].sum()


def test_the_workspace_cap_and_a_second_call_change_nothing(ctx):
    q, lv = noise_plane()
    E = 2 * q.shape[0] * q.shape[1]
    first = ctx.contour_polylines(q[None], lv)
    same_result(ctx.contour_polylines(q[None], lv), first, 'the second call')
    try:
        for rows in (1, 3, len(lv)):                                         # a group holds one range, three ranges, all ranges
            ctx.set_cpiece_workspace(rows * E * 4)
            same_result(ctx.contour_polylines(q[None], lv), first, 'a cap of %d ranges' % rows)
    finally:
        ctx.set_cpiece_workspace(DEFAULT_CAP)


def facade(q, y, x, lead=()):
    dims = tuple('d%d' % i for i in range(len(lead))) + ('latitude', 'longitude')
    c = {'latitude': y, 'longitude': x}
    c.update({'d%d' % i: np.arange(n) for i, n in enumerate(lead)})
    tr = xa.DataArray(q, dims, c, 'q')
    return xa.Contour2D(tr, np.ones(len(y)), {'X': 'longitude', 'Y': 'latitude'}, {'Y': 'latitude'}, dtype=q.dtype)


def same_nested(a, b, what=''):
    """the nested returns of two find_contours calls: the same nesting, arrays bit for bit, flags and windings equal"""
    if isinstance(a, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b), what
        for u, v in zip(a, b):
            same_nested(u, v, what)
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype == np.float64 and a.shape == b.shape and np.array_equal(bits(a), bits(b)), what
    else:
        assert type(a) is type(b) and a == b, what


def check_packed(packed, nested, lead):
    out, closed, winding = nested
    verts, voff, cl, wd, span = packed
    if not lead:
        out, closed, winding, span = [out], [closed], [winding], span[None]
    assert span.shape == (len(out), len(out[0]), 2) and int(voff[-1]) == verts.shape[0]
    npoly = 0
    for s in range(len(out)):
        for k in range(len(out[s])):
            a, b = int(span[s, k, 0]), int(span[s, k, 1])
            assert b - a == len(out[s][k]), (s, k)
            for p, v in zip(range(a, b), out[s][k]):
                assert np.array_equal(bits(verts[voff[p]:voff[p + 1]]), bits(v)), (s, k, p)
            assert cl[a:b].tolist() == list(closed[s][k]) and wd[a:b].tolist() == list(winding[s][k]), (s, k)
            npoly += b - a
    assert npoly == cl.size == wd.size == voff.size - 1


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['float64', 'float32'])
@pytest.mark.parametrize('periodic', [False, True], ids=['plain', 'periodic'])
def test_trace_contours_with_the_device_join_equals_find_contours(dtype, periodic):
    q, lv = noise_plane()
    q = q.astype(dtype)
    y, x = np.linspace(-80.0, 80.0, q.shape[0]), np.arange(q.shape[1]) * 9.0
    cm = facade(q, y, x)
    for index in (True, False):
        kw = dict(index=index, periodic=periodic)
        host = cm.find_contours(lv, return_closed=True, return_winding=True, **kw)
        dev = cm.trace_contours(lv, return_closed=True, return_winding=True, join='device', **kw)
        same_nested(dev, host, 'index=%s' % index)
        assert sum(len(p) for p in host[0]) > 30
        same_nested(cm.trace_contours(lv, join='device', **kw), cm.find_contours(lv, **kw), 'the lists alone')
        same_nested(cm.trace_contours(lv, return_closed=True, join='device', **kw), cm.find_contours(lv, return_closed=True, **kw), 'closed')
        # levels in descending order
        same_nested(cm.trace_contours(lv[::-1].copy(), return_winding=True, join='device', **kw),
                    cm.find_contours(lv[::-1].copy(), return_winding=True, **kw), 'descending levels')
        # packed, by either join, against the nested return; levels in a mixed order
        mixed = lv[[3, 0, 6, 1, 5, 2, 4]]
        nested = cm.find_contours(mixed, return_closed=True, return_winding=True, **kw)
        for join in ('host', 'device'):
            check_packed(cm.trace_contours(mixed, packed=True, join=join, **kw), nested, lead=False)


def test_a_stack_of_two_slabs_with_levels_per_slab():
    rng = np.random.default_rng(43)
    q = rng.standard_normal((2, 21, 30))
    q[1, 5:8, 10:14] = np.nan
    y, x = np.arange(21) * 1.5, np.arange(30) * 12.0
    cm = facade(q, y, x, lead=(2,))
    per = np.array([[0.7, -0.5, 0.1], [9.0, 0.0, -1.2]])                     # unsorted, per slab; one level above the field
    ctr = xa.DataArray(per, ('d0', 'contour'), {'d0': np.arange(2), 'contour': np.arange(3.0)}, 'q')
    for periodic in (False, True):
        host = cm.find_contours(ctr, return_closed=True, return_winding=True, periodic=periodic)
        dev = cm.trace_contours(ctr, return_closed=True, return_winding=True, periodic=periodic, join='device')
        same_nested(dev, host, 'periodic=%s' % periodic)
        assert len(host[0]) == 2 and len(host[0][0]) == 3 and host[0][1][0] == [] and len(host[0][0][0]) > 0
        check_packed(cm.trace_contours(ctr, periodic=periodic, join='device', packed=True), host, lead=True)


def test_the_barotropic_field_through_the_facade_and_trace_contour(baro):
    q, lat, lon = baro
    q = np.asarray(q, dtype=np.float64)
    cm = facade(q, np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64))
    lv = np.linspace(float(q.min()), float(q.max()), 9)[1:-1]
    for periodic in (False, True):
        host = cm.find_contours(lv, return_closed=True, return_winding=True, periodic=periodic)
        same_nested(cm.trace_contours(lv, return_closed=True, return_winding=True, periodic=periodic, join='device'), host, 'baro')
        check_packed(cm.trace_contours(lv, periodic=periodic, join='device', packed=True), host, lead=False)
    assert all(sum(abs(w) == 1 for w in ws) == 1 for ws in host[2])         # one |W| = 1 ring per level
    tr = xa.DataArray(q, ('latitude', 'longitude'), {'latitude': lat, 'longitude': lon}, 'q')
    a = xa.trace_contour(tr, ['latitude', 'longitude'], float(lv[3]), periodic=True, join='device')
    same_nested(a, xa.find_contour(tr, ['latitude', 'longitude'], float(lv[3]), periodic=True), 'find_contour')


def test_join_takes_two_values_and_a_plane_past_the_limit_names_the_host_join():
    q, lv = noise_plane()
    cm = facade(q, np.arange(33.0), np.arange(40.0))
    for bad in ('gpu', None, True, 'Device'):
        with pytest.raises(Exception, match='join'):
            cm.trace_contours(lv, index=True, join=bad)

    from xcontour_amd import core

    class Wide(object):                                                      # a lazy stack: only its shape is ever read
        _xc_lazy_stack, shape, dtype = True, (1, 1 << 15, 1 << 15), np.dtype(np.float32)
    core._check_device_join(1 << 15, (1 << 15) - 1)                          # 2 ny nx = 2^31 - 2^16: the largest plane of that height
    with pytest.raises(Exception, match="join='host'"):
        core._check_device_join(1 << 15, 1 << 15)
    with pytest.raises(nat.XContourHipError, match='2 ny nx < 2\\^31'):
        nat.Context.contour_polylines(None, Wide(), np.array([0.0]))         # refused from the shape alone: no context is touched
