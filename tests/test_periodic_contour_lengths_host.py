"""The periodic X direction of cal_contour_lengths / cal_local_contour_lengths without a GPU: the entry points and prototypes exist,
the facade rejects bad periods before it touches a device, and the numpy restatement (clength_periodic_ref) meets closed forms
and is additive over the seam cell column."""
import inspect

import numpy as np
import pytest

import clength_periodic_ref as PR
import clength_ref as CR
import local_clength_ref as LR
import xcontour_amd as xa
from xcontour_amd import _native as nat

NEW = ('xc_contour_lengths_periodic', 'xc_contour_lengths_periodic_dev', 'xc_local_contour_lengths_periodic',
       'xc_local_contour_lengths_periodic_dev')


def test_entry_points_and_prototypes_exist():
    lib = nat.load()
    for name in NEW:
        assert name in nat.PROTOTYPES and hasattr(lib, name)
        old = nat.PROTOTYPES[name.replace('_periodic', '')][1]
        new = nat.PROTOTYPES[name][1]
        assert list(new) == list(old[:8]) + [nat._f64] + list(old[8:])              # `double period` after xcoord
    for f in (nat.Context.contour_lengths, nat.Context.local_contour_lengths):
        assert inspect.signature(f).parameters['period'].default is None
    for f in (xa.Contour2D.cal_contour_lengths, xa.Contour2D.cal_local_contour_lengths):
        assert inspect.signature(f).parameters['periodic'].default is False


def _cm(lon, ny=5):
    q = xa.DataArray(np.zeros((ny, lon.size)), ('lat', 'lon'), {'lat': np.linspace(-40.0, 40.0, ny), 'lon': lon}, 'q')
    return xa.Contour2D(q, np.ones(ny), {'X': 'lon', 'Y': 'lat'}, {'Y': 'lat'})


@pytest.mark.parametrize('local', [False, True])
def test_facade_rejects_bad_periods_before_touching_a_device(local):
    lon = np.arange(0.0, 360.0, 45.0)                                                # 0 ... 315

    def call(cm, **kw):
        if local:
            return cm.cal_local_contour_lengths(3, **kw)
        return cm.cal_contour_lengths(np.array([0.5]), **kw)
    cm = _cm(lon)
    with pytest.raises(Exception, match='periodic=True needs latlon=True'):
        call(cm, periodic=True)
    for bad, text in ((0, 'periodic should be a finite, non-zero period'), (0.0, 'periodic should be a finite, non-zero period'),
                      (np.nan, 'periodic should be a finite, non-zero period'), (np.inf, 'periodic should be a finite, non-zero period'),
                      (-360.0, 'periodic=-360.0 runs against the X coordinate'), (315.0, 'periodic=315.0 is too short'),
                      (300, 'periodic=300 is too short'), ('ring', 'periodic should be False, True or the period')):
        for latlon in (False, True):
            with pytest.raises(Exception, match=text):
                call(cm, periodic=bad, latlon=latlon)
    with pytest.raises(Exception, match='periodic=360.0 runs against the X coordinate'):
        call(_cm(lon[::-1].copy()), periodic=360.0, latlon=True)                    # a descending longitude wants a negative period
    with pytest.raises(Exception, match='at least two columns'):
        call(_cm(lon[:1]), periodic=360.0, latlon=True)


def test_facade_rejects_a_window_wider_than_the_ring():
    cm = _cm(np.arange(0.0, 360.0, 45.0), ny=12)                                     # 8 columns
    with pytest.raises(Exception, match='window should not be wider than the periodic dim lon: 9 > 8'):
        cm.cal_local_contour_lengths({'lat': 3, 'lon': 9}, latlon=True, periodic=True)
    with pytest.raises(Exception, match='window should not be wider than the periodic dim lon: 9 > 8'):
        cm.cal_local_contour_lengths(9, periodic=360.0)


def test_period_handed_down_follows_the_coordinates_cast_chain():
    f = xa.Contour2D._x_period
    lon = np.arange(0.0, 360.0, 45.0).astype(np.float32)
    assert f(False, lon, True, 'f') is None and f(None, lon, False, 'f') is None
    assert f(True, lon, True, 'f') == float(np.float64(np.deg2rad(np.float32(360.0))))
    assert f(True, lon[::-1], True, 'f') == -float(np.float64(np.deg2rad(np.float32(360.0))))
    assert f(400.5, lon, True, 'f') == float(np.float64(np.deg2rad(np.float32(400.5))))
    assert f(400.1, lon, False, 'f') == 400.1


# ------------------------------------------------------------------ the restatement's helpers
def test_extend_and_tile_plane():
    q = np.arange(12.0).reshape(3, 4)
    x = np.array([0.0, 0.5, 1.5, 2.0])
    qe, xe = PR.extend_plane(q, x, 2.75)
    assert np.array_equal(qe, np.concatenate([q, q[:, :1]], axis=1)) and np.array_equal(xe, [0.0, 0.5, 1.5, 2.0, 2.75])
    qt, xt = PR.tile_plane(q, x, 2.75, 5)                                            # more than one lap to the left and right
    cols = [3, 0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3, 0]
    assert np.array_equal(qt, q[:, cols])
    assert np.array_equal(xt, [2.0 - 5.5, -2.75, -2.25, -1.25, -0.75, 0.0, 0.5, 1.5, 2.0, 2.75, 3.25, 4.25, 4.75, 5.5])
    qd, xd = PR.tile_plane(q, x[::-1].copy(), -2.75, 1)                              # descending coordinates, negative period
    assert np.array_equal(xd, [0.0 + 2.75, 2.0, 1.5, 0.5, 0.0, 2.0 - 2.75])
    assert PR.halo(9, 4) == 12 and PR.halo(8, 4) == 8 and PR.halo(3, 5) == 5
    for bad in (0.0, np.nan, -2.75, 2.0, 1.0):
        with pytest.raises(AssertionError):
            PR.extend_plane(q, x, bad)


# ------------------------------------------------------------------ closed forms
@pytest.mark.parametrize('seam', [0.5, 0.125])
def test_zonal_field_ring_closed_form(seam):
    """q = f(row) on a Cartesian ring with dyadic spacing: a level between two rows is one closed line of length |period| -- and
    |period| minus the seam cell's width without the wrap"""
    ny, nx = 9, 24
    q = np.repeat((np.arange(ny, dtype=np.float64) * 3.0)[:, None], nx, axis=1)
    y = np.arange(ny) * 0.25
    for sign in (1.0, -1.0):
        x = sign * (3.0 + np.arange(nx) * 0.5)
        period = sign * ((nx - 1) * 0.5 + seam)
        lv = np.array([0.7, 10.1, 22.5])
        tot, cnt = PR.contour_lengths(q, lv, y, x, period)
        plain, pcnt = CR.contour_lengths(q, lv, y, x)
        assert np.array_equal(tot, np.full(3, abs(period))) and np.array_equal(cnt, np.full(3, nx))
        assert np.array_equal(plain, np.full(3, abs(period) - seam)) and np.array_equal(pcnt, np.full(3, nx - 1))
        ft, fn = PR.contour_lengths_fast(q, lv, y, x, period)
        assert np.array_equal(ft, tot) and np.array_equal(fn, cnt)


@pytest.mark.parametrize('wx,sx', [(9, 1), (8, 3), (24, 23)])
def test_every_periodic_window_has_its_full_width(wx, sx):
    ny, nx, wy, sy = 20, 24, 7, 3
    q = np.repeat((np.arange(ny, dtype=np.float64) ** 1.5)[:, None], nx, axis=1)
    y, x = np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64)
    lv = PR.window_levels(q, (wy, wx), (sy, sx), float(nx), min_periods=1)
    nwx = LR.centres(nx, sx).size
    assert lv.shape == (7, nwx)
    tot, cnt = PR.local_contour_lengths(q, lv, y, x, float(nx), (wy, wx), (sy, sx))
    # the windows centred on column 0 and on the last centre (column nx-1 at strides 1 and 23) included: wx - 1 cells, no clipping
    assert np.array_equal(tot, np.full(tot.shape, wx - 1.0)) and np.array_equal(cnt, np.full(cnt.shape, wx - 1))
    clipped, _ = LR.local_contour_lengths(q, LR.window_levels(q, (wy, wx), (sy, sx), 1), y, x, (wy, wx), (sy, sx))
    assert clipped[0, 0] == wx - 1 - wx // 2                                         # what the seam stripe loses today


def test_periodic_window_means_keep_window_order():
    rng = np.random.default_rng(3)
    q = rng.standard_normal((6, 10)) * 10.0 ** rng.integers(-3, 4, (6, 10))
    q[2, 9] = np.nan
    lv = PR.window_levels(q, (3, 5), (2, 3), 10.0, min_periods=1)
    assert lv.shape == (3, 4)
    # window (1, 0): rows 1..3, columns 8, 9, 0, 1, 2 in that order
    assert lv[1, 0] == LR.sequential_mean(q[1:4][:, [8, 9, 0, 1, 2]], 1)
    assert lv[1, 3] == LR.sequential_mean(q[1:4][:, [7, 8, 9, 0, 1]], 1)
    assert lv[1, 1] == LR.sequential_mean(q[1:4, 1:6], 1)
    full = PR.window_levels(q, (3, 5), (2, 3), 10.0)                                 # min_periods = 15: only the NaN and the Y edges miss it
    assert np.isnan(full[0]).all() and np.isnan(full[1, [0, 3]]).all() and not np.isnan(full[1, 1:3]).any()


# ------------------------------------------------------------------ additivity
def test_periodic_is_plain_plus_the_seam_column_on_the_barotropic_field(baro):
    q, lat, lon = baro
    q = q.astype(np.float64)
    y, x = CR.plane_coords(lat, lon, True)
    period = float(np.float64(np.deg2rad(np.float32(360.0))))
    lv = np.linspace(q.min(), q.max(), 41)
    pt, pn = PR.contour_lengths_fast(q, lv, y, x, period, True)
    t0, n0 = CR.contour_lengths_fast(q, lv, y, x, True)
    seam_q = np.stack([q[:, -1], q[:, 0]], axis=1)
    seam_x = np.array([x[-1], x[0] + period])
    t1, n1 = CR.contour_lengths_fast(seam_q, lv, y, seam_x, True)
    assert np.array_equal(pn, n0 + n1) and n1.sum() > 0
    tot = np.nan_to_num(t0) + np.nan_to_num(t1)
    ok = pn > 0
    assert np.array_equal(np.isnan(pt), ~ok)
    assert np.max(np.abs(pt[ok] - tot[ok]) / pt[ok]) <= 1e-12
    # every contour that crosses the seam is longer by its seam segments
    assert (pt[n1 > 0] > t0[n1 > 0]).all()
