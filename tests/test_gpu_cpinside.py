"""Context.contour_piece_interiors and Contour2D.cal_integral_inside_pieces (K18) on the GPU, against cpinside_ref.piece_interiors on
Context.contour_segments of the same input -- integers equal, sums bit for bit -- and against the library's own K13 and K17: the row of
the main ring is K17 with select='main', a range of one piece is K17 with select='all', the key fields are cal_contour_pieces'."""
import numpy as np
import pytest

import cpinside_ref as PR
import xcontour_amd as xa
import xcontour_oracle as O

pytestmark = pytest.mark.gpu


def per_range(pc, table):
    off = np.concatenate([[0], np.cumsum(pc.ravel().astype(np.int64))])
    return [table[a:b] for a, b in zip(off[:-1], off[1:])]


def against_the_restatement(ctx, q, lv, periodic, flip=False, w=None, f=None):
    pc, tab = ctx.contour_piece_interiors(q, lv, w=w, f=f, periodic=periodic, flip=flip)
    assert tab.dtype == ctx.PIECE_INTERIOR_DTYPE and pc.shape == (q.shape[0], len(lv))
    cnt, ef, et, pts = ctx.contour_segments(q, lv, periodic=periodic)
    ref = PR.piece_interiors(cnt.ravel(), ef, et, pts, q.shape[1], q.shape[2], int(periodic), flip=int(flip), ncont=len(lv), w=w, f=f)
    got = per_range(pc, tab)
    assert [g.size for g in got] == [t.size for t in ref]
    for r, (g, t) in enumerate(zip(got, ref)):
        assert PR.differences(g.astype(PR.DTYPE), t) == [], 'range %d' % r
    return pc, tab, got


def blocked_noise(nslab, ny, nx, seed):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((nslab, ny, nx)) + np.linspace(-2.0, 2.0, ny)[None, :, None]
    q[0, ny // 3:ny // 3 + 2, nx // 4:nx // 4 + 3] = np.nan
    q[-1, ny - 4, nx - 1] = np.nan
    q[-1, 0, 0] = np.nan
    return q


@pytest.mark.parametrize('periodic', [False, True], ids=['plain', 'ring'])
@pytest.mark.parametrize('nx', [63, 64, 65])
def test_nan_blocked_noise_a_batch_of_slabs_and_two_calls_in_a_row(ctx, nx, periodic):
    ny = 40
    q = blocked_noise(3, ny, nx, 120 + nx)
    lv = np.array([-0.8, 0.0, 0.9])
    rng = np.random.default_rng(121)
    w, f = rng.random((3, ny, nx)) + 0.5, rng.standard_normal((3, ny, nx)).astype(np.float32)
    pc, tab, _ = against_the_restatement(ctx, q, lv, periodic, flip=True, w=w, f=f)
    pc2, tab2 = ctx.contour_piece_interiors(q, lv, w=w, f=f, periodic=periodic, flip=True)
    assert pc2.tobytes() == pc.tobytes() and tab2.tobytes() == tab.tobytes()
    keep = ctx.max_batch_bytes
    try:
        ctx.max_batch_bytes = 1                                              # one slab per batch
        pc3, tab3 = ctx.contour_piece_interiors(q, lv, w=w, f=f, periodic=periodic, flip=True)
    finally:
        ctx.max_batch_bytes = keep
    assert pc3.tobytes() == pc.tobytes() and tab3.tobytes() == tab.tobytes()
    assert (tab['closed'] & (tab['n_in'] > 5)).any() and (~tab['closed']).any()


def test_the_2_x_3_plane_and_a_resident_tracer(ctx):
    q = np.zeros((1, 6, 7))
    q[0, 2:4, 1:4] = 1.0
    w = np.arange(42, dtype=np.float64).reshape(6, 7)
    _, tab, _ = against_the_restatement(ctx, q, np.array([0.5]), False, w=w)
    assert tab['n_in'].tolist() == [6] and tab['nseg'].tolist() == [10] and tab['sum_w'].tolist() == [w[2:4, 1:4].sum()]
    assert np.isnan(tab['sum_wf']).all()
    ctx.keep_resident(q)
    try:
        _, again, _ = against_the_restatement(ctx, q, np.array([0.5]), False, w=w)
    finally:
        ctx.release_resident(q)
    assert again.tobytes() == tab.tobytes()
    assert ctx.contour_piece_interiors(q, np.array([7.0]))[1].size == 0


@pytest.fixture(scope='module')
def case(baro):
    q, lat, lon = (np.asarray(a) for a in baro)
    q = q.astype(np.float64)
    c = {'latitude': lat, 'longitude': lon}
    dA = np.asarray(O.cell_area(lat, lon), dtype=np.float64)
    cm = xa.Contour2D(xa.DataArray(q, ('latitude', 'longitude'), c, 'q'), xa.DataArray(dA, ('latitude', 'longitude'), c, 'dA'),
                      {'X': 'longitude', 'Y': 'latitude'}, {'Y': 'latitude'}, dtype=np.float64)
    lv = np.sort(np.concatenate([np.quantile(q, [0.2, 0.35, 0.5, 0.65, 0.8]), [q[40, 100], float(q.max()) - 1e-9]]))
    return dict(q=q, lat=lat, lon=lon, dA=dA, cm=cm, lv=lv, ascends=bool(lat[-1] >= lat[0]))


@pytest.mark.parametrize('flip', [False, True])
def test_the_barotropic_field_periodic_and_the_identities_with_k13_and_k17(ctx, case, flip):
    q, dA, lv = case['q'][None], case['dA'], case['lv']
    f = q * q
    pc, tab, got = against_the_restatement(ctx, q, lv, True, flip=flip, w=dA, f=f)
    # the key fields are K13's
    pc13, tab13 = ctx.contour_pieces(q, lv, case['lat'].astype(np.float64), case['lon'].astype(np.float64), period=360.0)
    assert np.array_equal(pc, pc13)
    for k in ('first_edge', 'nseg', 'closed', 'winding'):
        assert np.array_equal(tab[k], tab13[k]), k
    # the row of the main ring is K17 with select='main'
    over = ctx.contour_overturning(q, lv, periodic=True, select='main')
    mfe = over[4][0]
    n17, sw17, swf17 = ctx.contour_interior(q, lv, w=dA, f=f, periodic=True, select='main', flip=flip)
    seen = 0
    for k, g in enumerate(got):
        if mfe[k] < 0:
            continue
        row = g[g['first_edge'] == mfe[k]]
        assert row.size == 1 and row['n_in'][0] == n17[0, k], k
        assert row['sum_w'].tobytes() == sw17[0, k:k + 1].tobytes() and row['sum_wf'].tobytes() == swf17[0, k:k + 1].tobytes(), k
        seen += 1
    assert seen >= 4
    # a range with exactly one piece is K17 with select='all'
    nall, swall, swfall = ctx.contour_interior(q, lv, w=dA, f=f, periodic=True, select='all', flip=flip)
    single = [k for k, g in enumerate(got) if g.size == 1 and g['closed'][0] and g['winding'][0] != 0]   # (K17 flips such a ring as K18 does)
    assert single, 'no level with a single ring'
    for k in single:
        g = got[k]
        assert g['n_in'][0] == nall[0, k] and g['sum_w'].tobytes() == swall[0, k:k + 1].tobytes() and g['sum_wf'].tobytes() == swfall[0, k:k + 1].tobytes()
    assert any((g['closed'] & (g['winding'] == 0)).any() for g in got), 'nothing shed at any level'


def test_the_facade_lines_up_with_cal_contour_pieces_in_caller_order(case):
    cm, lv, q, dA = case['cm'], case['lv'], case['q'], case['dA']
    mixed = np.array([lv[3], np.nan, lv[0], lv[5]])
    g = xa.DataArray(q * q, ('latitude', 'longitude'), {'latitude': case['lat'], 'longitude': case['lon']}, 'q2')
    out = cm.cal_integral_inside_pieces(mixed, integrand=g, periodic=True)
    pieces = cm.cal_contour_pieces(mixed, periodic=360.0)
    assert len(out) == 4 and out[1].size == 0 and pieces[1].size == 0
    assert out[0].dtype.names == ('first_edge', 'nseg', 'closed', 'winding', 'nodes', 'area', 'integral')
    for a, b in zip(out, pieces):
        for k in ('first_edge', 'nseg', 'closed', 'winding'):
            assert np.array_equal(a[k], b[k]), k
    flip = not case['ascends']                                               # side='upper'
    pc, tab = cm.ctx.contour_piece_interiors(q[None], lv[[0, 3, 5]], w=dA, f=(q * q)[None], periodic=True, flip=flip)
    raw = per_range(pc, tab)
    for a, b in zip((out[2], out[0], out[3]), raw):
        assert a['nodes'].tobytes() == b['n_in'].tobytes() and a['area'].tobytes() == b['sum_w'].tobytes()
        assert a['integral'].tobytes() == b['sum_wf'].tobytes()
    bare = cm.cal_integral_inside_pieces(mixed, periodic=True, side='lower')
    assert bare[0].dtype.names == ('first_edge', 'nseg', 'closed', 'winding', 'nodes', 'area')
    main = out[0][out[0]['winding'] != 0][0]
    other = bare[0][bare[0]['winding'] != 0][0]
    assert main['nodes'] + other['nodes'] == q.size                          # the two sides of the ring that goes round
    shed = out[3]['closed'] & (out[3]['winding'] == 0)
    assert shed.any() and np.array_equal(out[3]['nodes'][shed], bare[3]['nodes'][shed])   # `side` leaves the other rings alone
    with pytest.raises(Exception, match='side'):
        cm.cal_integral_inside_pieces(mixed, periodic=True, side='north')


def test_a_descending_latitude_with_side_and_a_leading_dim():
    rng = np.random.default_rng(44)
    q = rng.standard_normal((3, 9, 12))
    q[:, 4:] += 3.0
    y, x = np.arange(9) * 1.5 - 6.0, np.arange(12) * 30.0
    lv = np.array([2.1, -0.8, 1.5, np.nan, 0.1])
    dA = rng.random((9, 12)) + 0.5
    res = {}
    for name, yc in (('up', y), ('down', y[::-1].copy())):
        c = {'latitude': yc, 'longitude': x, 'd0': np.arange(3)}
        cm = xa.Contour2D(xa.DataArray(q, ('d0', 'latitude', 'longitude'), c, 'q'), xa.DataArray(dA, ('latitude', 'longitude'), c, 'dA'),
                          {'X': 'longitude', 'Y': 'latitude'}, {'Y': 'latitude'}, dtype=np.float64)
        for side in ('upper', 'lower'):
            out = cm.cal_integral_inside_pieces(lv, periodic=True, side=side)
            assert len(out) == 3 and all(len(o) == 5 and o[3].size == 0 for o in out)
            res[name, side] = out
            flip = (side == 'upper') != (name == 'up')
            order = np.argsort(np.where(np.isnan(lv), np.inf, lv), kind='stable')
            pc, tab = cm.ctx.contour_piece_interiors(q, np.where(np.isnan(lv), np.inf, lv)[order], w=dA, periodic=True, flip=flip)
            raw = per_range(pc, tab)
            for s in range(3):
                for j, k in enumerate(order):
                    assert out[s][k]['nodes'].tobytes() == raw[s * 5 + j]['n_in'].tobytes()
                    assert out[s][k]['area'].tobytes() == raw[s * 5 + j]['sum_w'].tobytes()
    # the same rows of the plane: 'upper' on the ascending coordinate is 'lower' on the descending one
    for s in range(3):
        for k in range(5):
            assert res['up', 'upper'][s][k].tobytes() == res['down', 'lower'][s][k].tobytes()
