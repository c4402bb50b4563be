"""Contour2D.cal_contour_folds (K24) on the GPU, through the facade, against PUBLIC calls only: on NaN-free fields everything it returns
is rebuilt in numpy from cal_integral_inside_contours(..., return_mask=True) -- the transitions of the mask down a column are the
crossing flags -- and cal_contour_overturning (the rows).  Integers equal; the sums bit for bit math.fsum (dA and the integrands here
have exponents far inside every window); the derived centroids bit for bit the facade's formulas restated."""
import math

import numpy as np
import pytest

import cfold_ref as FR
import xcontour_amd as xa

pytestmark = pytest.mark.gpu


def contour2d(q, lat, lon, dA, lead=()):
    c = {'latitude': lat, 'longitude': lon}
    c.update({d: np.arange(n) for d, n in lead})
    dims = tuple(d for d, _ in lead) + ('latitude', 'longitude')
    return xa.Contour2D(xa.DataArray(q, dims, c, 'q'), xa.DataArray(dA, ('latitude', 'longitude'), {'latitude': lat, 'longitude': lon}, 'dA'),
                        {'X': 'longitude', 'Y': 'latitude'}, {'Y': 'latitude'}, dtype=np.float64), c, dims


def fold_x(col, xg, period):
    nx = xg.size
    if period is None:
        return np.interp(col, np.arange(nx), xg)
    k = np.floor(col / nx)
    return np.interp(col - k * nx, np.arange(nx + 1), np.append(xg, xg[0] + period)) + k * period


def rebuilt(mask, ncross, y_lo, y_hi, dA, g, yg, xg, period, gap):
    """one (slab, level): mask bool (ny, nx), K16's columns -> (event labels (nx,), the rows of the facade's table as dicts)"""
    ny, nx = mask.shape
    X = mask[1:] != mask[:-1]
    assert np.array_equal(X.sum(axis=0), ncross)
    P = mask ^ mask[:1]
    label = np.full(nx, -1, dtype=np.int32)
    rows = []
    for j, cols in enumerate(FR.runs(ncross >= 3, gap, period is not None)):
        cw, ce = cols[0], cols[-1]
        label[cols] = j
        T = {k: ([], []) for k in ('area', 'mx', 'my', 'integral')}
        for c in cols:
            r = np.flatnonzero(X[:, c])
            lo, hi = int(r[0]), int(r[-1])
            for row in range(lo + 1, hi + 1):
                t = int(P[row, c] ^ P[lo + 1, c])
                a = dA[row, c]
                T['area'][t].append(a); T['mx'][t].append(a * np.float64((c - cw) % nx)); T['my'][t].append(a * np.float64(row))
                if g is not None:
                    T['integral'][t].append(a * g[row, c])
        S = {k: [math.fsum(v[0]), math.fsum(v[1])] for k, v in T.items()}
        e = dict(c_west=cw, c_east=ce, ncol=len(cols), ncross_max=int(ncross[cols].max()), width=(ce - cw) % nx + 1, x_west=xg[cw],
                 x_east=xg[ce], y_lo=y_lo[cols].min(), y_hi=y_hi[cols].max())
        lean = []
        for t, name in enumerate(('_under', '_over')):
            e['nodes' + name], e['area' + name] = len(T['area'][t]), S['area'][t]
            e['integral' + name] = S['integral'][t] if g is not None else np.nan
            with np.errstate(all='ignore'):
                mcol, mrow = np.float64(S['mx'][t]) / np.float64(S['area'][t]), np.float64(S['my'][t]) / np.float64(S['area'][t])
            e['cy' + name] = float(np.interp(mrow, np.arange(ny), yg))
            e['cx' + name] = float(fold_x(np.float64(cw) + mcol, xg, period))
            lean.append(mcol)
        d = lean[1] - lean[0]
        e['orientation'] = 0 if (S['area'][0] == 0 or S['area'][1] == 0 or np.isnan(d)) else int(np.sign(d))
        rows.append(e)
    return label, rows


def same(a, b):
    a, b = np.float64(a), np.float64(b)
    return (np.isnan(a) and np.isnan(b)) or a.tobytes() == b.tobytes()


def check(cm, lv, q, dA, yg, xg, periodic, select, gap, g=None, gda=None):
    """q (nslab, ny, nx), lv in the caller's order; -> the events of every (slab, level)"""
    period = 360.0 if periodic else None
    cols, events = cm.cal_contour_folds(lv, integrand=gda, periodic=periodic, select=select, gap=gap)
    ins = cm.cal_integral_inside_contours(lv, integrand=gda, periodic=periodic, select=select, return_mask=True)
    over = cm.cal_contour_overturning(lv, periodic=periodic, select=select)
    assert list(cols) == ['ncross', 'y_lo', 'y_hi', 'event'] and cols['event'].values.dtype == np.int32
    for k in ('ncross', 'y_lo', 'y_hi'):
        assert cols[k].values.tobytes() == over[k].values.tobytes() and cols[k].dims == over[k].dims, k
    nslab, N = q.shape[0], len(lv)
    mask = ins['mask'].values.reshape(nslab, N, *q.shape[1:])
    nc, ylo, yhi, lab = (cols[k].values.reshape(nslab, N, -1) for k in ('ncross', 'y_lo', 'y_hi', 'event'))
    ev = events if q.shape[0] > 1 or isinstance(events[0], list) else [events]
    for s in range(nslab):
        for k in range(N):
            label, rows = rebuilt(mask[s, k], nc[s, k], ylo[s, k], yhi[s, k], dA, None if g is None else g[s], yg, xg, period, gap)
            assert np.array_equal(lab[s, k], label), (s, k)
            tab = ev[s][k]
            assert tab.dtype.names == tuple(n for n, _ in xa.Contour2D.FOLD_FIELDS) and tab.size == len(rows), (s, k)
            for e, row in zip(tab, rows):
                for name, want in row.items():
                    if tab.dtype[name].kind == 'f':
                        assert same(e[name], want), (s, k, name, e[name], want)
                    else:
                        assert int(e[name]) == int(want), (s, k, name, e[name], want)
    return ev


def hand_built():
    m = FR.plane(24, 48, 16)
    FR.hook(m, (10, 11, 12, 13, 14), 15, 5, 9, 16)
    FR.hook(m, (46, 47, 0, 1), 2, 3, 7, 16)
    FR.hook(m, (30, 31), 29, 8, 10, 16)
    FR.hook(m, (33, 34), 35, 4, 6, 16)
    m[2:4, 20:23] = 1                                                        # a detached blob: folded under 'all' only
    return FR.field(m)


@pytest.mark.parametrize('descending', [False, True], ids=['lat up', 'lat down'])
def test_a_hand_built_plane_every_select_and_gap(descending):
    q = hand_built()
    lat, lon = np.linspace(-69.0, 69.0, 24), np.arange(48) * 7.5
    if descending:
        lat = lat[::-1].copy()
    rng = np.random.default_rng(31)
    dA = rng.uniform(0.5, 2.0, q.shape)
    cm, c, dims = contour2d(q, lat, lon, dA)
    g = rng.standard_normal((1,) + q.shape)
    gda = xa.DataArray(g[0], dims, c, 'g')
    lv = np.array([0.5])
    main = check(cm, lv, q[None], dA, lat, lon, True, 'main', 0, g, gda)[0][0]
    assert main['c_west'].tolist() == [10, 30, 33, 46] and main['c_east'].tolist() == [14, 31, 34, 1] and main['width'].tolist() == [5, 2, 2, 4]
    assert set(main['orientation'].tolist()) <= {-1, 1}                      # (rectangular tongues: the lean is the weights' alone)
    assert (main['x_east'][3], main['x_west'][3]) == (7.5, 345.0) and 345.0 < main['cx_under'][3] < 360.0 + 7.5
    assert ((main['y_lo'] < main['y_hi']).all() and (main['cy_under'] > main['y_lo']).all() and (main['cy_under'] < main['y_hi']).all())
    bridged = check(cm, lv, q[None], dA, lat, lon, True, 'main', 1, g, gda)[0][0]
    assert bridged['c_west'].tolist() == [10, 30, 46] and bridged['ncol'].tolist() == [5, 4, 4]
    every = check(cm, lv, q[None], dA, lat, lon, True, 'all', 0)[0][0]
    assert every['c_west'].tolist() == [10, 20, 30, 33, 46] and np.isnan(every['integral_under']).all()
    plain = check(cm, lv, q[None], dA, lat, lon, False, 'all', 0)[0][0]
    assert plain['c_west'].tolist() == [0, 10, 20, 30, 33, 46] and plain['c_east'].tolist() == [1, 14, 22, 31, 34, 47]


def pv_like(ny=61, nx=120, mirror=False):
    """a zonal gradient displaced by two tilted Gaussian tongues, steep enough to overturn: one leans east, one west"""
    y, x = np.meshgrid(np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing='ij')
    q = y.copy()
    for x0, k in ((30.0, 1.5), (85.0, -1.5)):
        q -= 12.0 * np.exp(-(((x - x0 - k * (y - 30.0)) / 8.0) ** 2))
    return q[:, ::-1].copy() if mirror else q


def test_a_pv_like_field_with_tilted_tongues_two_slabs_levels_out_of_order_and_its_mirror_image():
    q = np.stack([pv_like(), pv_like(mirror=True)])
    ny, nx = q.shape[1:]
    lat, lon = np.linspace(0.0, 90.0, ny), np.arange(nx) * 3.0
    dA = np.cos(np.deg2rad(lat))[:, None] * np.ones(nx) * 1.0e9 + 1.0
    cm, c, dims = contour2d(q, lat, lon, dA, lead=(('time', 2),))
    g = q * q
    gda = xa.DataArray(g, dims, c, 'g')
    lv = np.array([27.3, 22.6, np.nan, 31.9, 25.2])
    ev = check(cm, lv, q, dA, lat, lon, True, 'main', 0, g, gda)
    assert all(ev[s][2].size == 0 for s in (0, 1))                          # the NaN level
    found = sum(ev[0][k].size for k in range(5))
    assert found >= 4 and {int(o) for k in range(5) for o in ev[0][k]['orientation']} == {-1, 1}
    # the mirror image: every event again, leaning the other way
    for k in (0, 1, 3, 4):
        a, b = ev[0][k], ev[1][k]
        assert a.size == b.size
        for e in a:
            m = b[b['c_west'] == nx - 1 - e['c_east']]
            assert m.size == 1 and m['c_east'][0] == nx - 1 - e['c_west'] and m['orientation'][0] == -e['orientation']
            assert m['nodes_under'][0] == e['nodes_under'] and m['nodes_over'][0] == e['nodes_over']
    check(cm, lv, q, dA, lat, lon, True, 'all', 3)
    check(cm, lv[[1, 0]], q, dA, lat, lon, False, 'all', 0)


def test_arguments_that_are_refused():
    q = hand_built()
    lat, lon = np.linspace(-69.0, 69.0, 24), np.arange(48) * 7.5
    cm, _, _ = contour2d(q, lat, lon, np.ones(q.shape))
    lv = np.array([0.5])
    for gap in (-1, 1.5, True, '1', 48, None):
        with pytest.raises(Exception):
            cm.cal_contour_folds(lv, periodic=True, gap=gap)
    for kw in (dict(select='main'), dict(select='circumpolar'), dict(periodic=True, select='largest')):
        with pytest.raises(Exception):
            cm.cal_contour_folds(lv, **kw)
    cols, events = cm.cal_contour_folds(lv, periodic=True, gap=47)           # every cyclic gap bridged: one event from the smallest folded column
    assert events[0]['c_west'].tolist() == [0] and events[0]['c_east'].tolist() == [47] and events[0]['ncol'].tolist() == [13]
