"""The restatement of K21 (cpprops_ref.piece_props: sets of nodes and math.fsum) and an independent one of the kernels' accumulation
(cpprops_ref.scan_props: chunks, private gathering, hand-over at state changes and chunk ends, the fold along parents), on the CPU -- no
GPU.  The two must agree on every hand-built plane of cptree_cases, on noise and on the barotropic field; five broken variants each fail
the case named for them; the inputs of the GPU tests hold what those tests are there for; and the host parts of
Contour2D.cal_contour_piece_props (moment planes, centroid formula, the fold of the gross extremum) equal straightforward loops."""
import numpy as np
import pytest

import cplabel_ref as LR
import cpprops_ref as QR
import cptree_cases as CS
import cptree_ref as TR
from test_cplabel_host import PLANES
from test_cptree_host import records
from xcontour_amd.core import Contour2D


def scaled(rng, shape, dtype=np.float64):
    v = np.ldexp(rng.uniform(1.0, 2.0, shape), rng.integers(-20, 20, shape)) * rng.choice([-1.0, 1.0], shape)
    return v.astype(dtype)


def inputs(seed, nslab, ny, nx, nf=3):
    rng = np.random.default_rng(seed)
    return dict(w=scaled(rng, (ny, nx)), fields=QR.field_set(rng, nf, nslab, ny, nx, scaled), x=QR.integer_x(rng, nslab, ny, nx))


def agree(rec, flip=0, rows=None, **kw):
    tables, want = QR.piece_props(*rec, flip=flip, **kw)
    got = QR.scan_props(*rec, flip=flip, rows=rows, **kw)
    for r, (a, b) in enumerate(zip(got, want)):
        assert QR.differences(a, b) == [], 'range %d' % r
    return tables, want


def caught(rec, wrong, flip=0, **kw):
    _, want = QR.piece_props(*rec, flip=flip, **kw)
    return any(QR.differences(a, b) for a, b in zip(QR.scan_props(*rec, flip=flip, wrong=wrong, **kw), want))


@pytest.mark.parametrize('flip', [0, 1])
@pytest.mark.parametrize('name, q, periodic', PLANES, ids=[p[0] for p in PLANES])
def test_the_accumulation_is_the_set_rule_on_every_hand_built_plane(name, q, periodic, flip):
    (t,), (p,) = agree(records(q, periodic), flip=flip, **inputs(q.size, 1, *q.shape))
    assert np.isnan(p['net'][~t['closed']]).all() and np.isfinite(p['net'][t['closed']]).all()


@pytest.mark.parametrize('rows', [1, 5])
def test_any_chunk_length_gives_the_same_sums(rows):
    for q, periodic in ((CS.stacked_siblings(), 0), (CS.bands(), 1), (CS.open_beside_nan(True), 0)):
        for flip in (0, 1):
            agree(records(q, periodic), flip=flip, rows=rows, **inputs(3, 1, *q.shape))


@pytest.mark.parametrize('periodic', [False, True], ids=['plain', 'ring'])
def test_the_accumulation_is_the_set_rule_on_smooth_noise(periodic):
    q = CS.smooth_noise(24, 63, 63)
    q[5:8, 7:9] = np.nan
    lv = np.linspace(-1.8, 1.8, 7)
    for flip in (0, 1):
        tables, _ = agree(records(q, periodic, lv), flip=flip, ncont=7, **inputs(7, 1, 24, 63, nf=5))
    assert max(int(t['depth'].max()) for t in tables if t.size) >= 1 and LR.scan_geometry(24) == (16, 2)


def test_the_accumulation_is_the_set_rule_on_the_barotropic_field(baro):
    q = baro[0].astype(np.float64)
    lv = np.quantile(q, [0.1, 0.3, 0.5, 0.7, 0.9])
    kw = inputs(11, 1, *q.shape, nf=2)
    kw['x'] = q[None]
    deep = 0
    for flip in (0, 1):
        tables, _ = agree(records(q, True, lv), flip=flip, ncont=5, **kw)
        deep = max(deep, max(int(t['depth'].max()) for t in tables if t.size))
    assert deep >= 1


# ------------------------------------------------------------------ five broken variants, each caught by its case
def test_a_scan_that_does_not_flush_at_the_chunk_end_is_caught_by_a_ring_over_two_chunks():
    q = CS.long_walk(True)                                                   # 600 rows: 32 chunks, the block spans them all
    assert LR.scan_geometry(600)[1] == 32 and caught(records(q, 1), 'no flush at the chunk end', **inputs(1, 1, *q.shape))
    assert not caught(records(q, 1), None, **inputs(1, 1, *q.shape))


def test_a_fold_that_reaches_the_parent_only_is_caught_by_a_chain():
    q = CS.chain(13)
    assert caught(records(q, 0), 'fold reaches the parent only', **inputs(2, 1, 13, 13))
    assert not caught(records(CS.two_blobs(), 0), 'fold reaches the parent only', **inputs(2, 1, 12, 6))   # (no grandchild there)


def test_a_tie_that_takes_the_last_node_is_caught_by_integer_values():
    q = CS.stacked_siblings()
    kw = inputs(4, 1, *q.shape)
    (t,), (p,) = agree(records(q, 0), **kw)
    lab = LR.labels_of_masks(TR.piece_tree(*records(q, 0), return_masks=True)[1][0], q.shape)
    assert any(((lab == k) & (kw['x'][0] == p['x_max'][k])).sum() > 1 for k in range(t.size) if p['x_max'][k] != 0)
    assert caught(records(q, 0), 'tie takes the last node', **kw)


def test_a_nan_that_wins_the_extremum_is_caught():
    q = CS.one_node()
    kw = inputs(5, 1, *q.shape)
    kw['x'][0, 2, 3] = np.nan                                                # the ring's only node: NaN, -1
    (t,), (p,) = agree(records(q, 0), **kw)
    assert np.isnan(p['x_min'][0]) and p['at_min'][0] == -1
    q = CS.two_blobs()
    kw = inputs(5, 1, *q.shape)
    kw['x'][0, 7, 2] = np.nan
    assert caught(records(q, 0), 'NaN wins the extremum', **kw)


def test_a_state_minus_one_that_accumulates_is_caught():
    q = CS.one_node()
    assert caught(records(q, 0), 'state -1 accumulates', **inputs(6, 1, *q.shape))


def test_signed_zeros_infinities_and_nan_terms_in_the_set_rule():
    q = CS.chain(13)
    kw = inputs(8, 1, 13, 13)
    kw['x'][0] = 1.0
    kw['x'][0, 6, 6], kw['x'][0, 5, 5], kw['x'][0, 5, 6] = np.nan, 0.0, -0.0
    kw['fields'][0][0, 6, 6] = np.inf
    kw['fields'][2][0, 5, 5] = np.nan
    (t,), (p,) = agree(records(q, 0), **kw)
    o = np.argsort(t['n_in'])                                                # innermost first: a chain
    assert np.isnan(p['net'][o[0], 0]) and np.isfinite(p['net'][o[1:], 0]).all() and np.isnan(p['gross'][:, 0]).all()
    assert np.isfinite(p['net'][:, 2]).all() and np.isnan(p['x_min'][o[0]]) and p['at_min'][o[0]] == -1
    assert p['x_min'][o[1]] == 0 and np.signbit(p['x_min'][o[1]]) and p['at_min'][o[1]] == 5 * 13 + 6


# ------------------------------------------------------------------ the inputs of the GPU tests hold what those tests are there for
def test_the_inputs_of_the_gpu_tests():
    import test_gpu_cptree_records as K19
    for periodic in (0, 1):
        q, rec, ny, nx = K19.noise_case(periodic)
        tabs = TR.piece_tree(*rec, ny, nx, periodic, ncont=4)
        assert max(int(t['depth'].max()) for t in tabs if t.size) >= 1 and any((~t['closed']).any() for t in tabs)
    assert max(int(t['depth'].max()) for t in TR.piece_tree(*records(CS.chain(13), 0))) >= 2
    assert [LR.scan_geometry(n)[1] for n in (6, 17, 24, 83, 513, 600)] == [1, 2, 2, 6, 31, 32]


# ------------------------------------------------------------------ the host parts of the facade
def loop_planes(yg, xg, latlon, period):
    out = []
    for k in range(2 if (not latlon and period is None) else 3):
        p = np.empty((yg.size, xg.size))
        for r, y in enumerate(yg):
            for c, x in enumerate(xg):
                if latlon:
                    la, lo = np.deg2rad(y), np.deg2rad(x)
                    p[r, c] = (np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la))[k]
                elif period is None:
                    p[r, c] = (y, x)[k]
                else:
                    a = 2 * np.pi * (x - xg[0]) / period
                    p[r, c] = (y, np.cos(a), np.sin(a))[k]
        out.append(p)
    return out


@pytest.mark.parametrize('latlon, period', [(True, 360.0), (False, 360.0), (False, None)], ids=['latlon', 'periodic', 'plain'])
def test_the_moment_planes_and_the_centroid_of_a_blob_across_the_seam(latlon, period):
    yg, xg = np.linspace(-40.0, 40.0, 9), np.arange(0.0, 360.0, 30.0)        # 12 columns, the seam between 330 and 0
    planes = Contour2D._moment_planes(yg, xg, latlon, period)
    for a, b in zip(planes, loop_planes(yg, xg, latlon, period)):
        assert np.array_equal(a, b)
    blob = np.zeros((9, 12), dtype=bool)
    blob[3:6, [10, 11, 0, 1]] = True                                         # columns 300, 330, 0, 30: its centre lies on the seam
    dA = np.cos(np.deg2rad(yg))[:, None] * np.ones((9, 12))
    m = [np.array([float(np.sum((dA * p)[blob]))]) for p in planes]
    area = np.array([float(dA[blob].sum())])
    cy, cx = Contour2D._centroid_of(m, area, latlon, period, float(xg[0]))
    assert abs(cy[0]) < 1e-9
    if period is not None:
        assert cx[0] > 330.0 or cx[0] < 30.0, 'the centroid longitude lies inside the blob'
        assert min(abs(cx[0] - 345.0), abs(cx[0] - 345.0 + 360.0)) < 1e-9
    else:
        assert abs(cx[0] - 165.0) < 1e-9                                     # a plain plane knows no seam: the mean of the columns
    z = [np.zeros(1) for _ in m]
    assert all(np.isnan(v[0]) for v in Contour2D._centroid_of(z, np.zeros(1), latlon, period, 0.0))
    n = [np.full(1, np.nan) for _ in m]
    assert all(np.isnan(v[0]) for v in Contour2D._centroid_of(n, area, latlon, period, 0.0))


def test_the_gross_extremum_of_a_chain_sits_in_a_grandchild():
    # rows: 0 the root, 1 its child, 2 the grandchild, 3 a second root with a child 4; 5 an open piece
    parent = np.array([-1, 0, 1, -1, 3, -1])
    depth = np.array([0, 1, 2, 0, 1, 0])
    v = np.array([5.0, np.nan, -3.0, 0.0, -0.0, np.nan])
    at = np.array([40, -1, 77, 9, 12, -1])
    for largest in (False, True):
        gv, ga = Contour2D._gross_extrema(parent, depth, v, at, largest)
        want_v, want_a = v.copy(), at.copy()
        for p in range(6):                                                   # the straightforward loop: every ring over its subtree
            best = None
            for c in range(6):
                q = c
                while q >= 0 and q != p:
                    q = parent[q]
                if q != p or at[c] < 0:
                    continue
                k = QR.order_key(v[c])
                k = -k if largest else k
                if best is None or (k, at[c]) < best[:2]:
                    best = (k, at[c], v[c])
            if best is not None:
                want_v[p], want_a[p] = best[2], best[1]
        assert QR.same_bits(gv, want_v) and np.array_equal(ga, want_a)
    gv, ga = Contour2D._gross_extrema(parent, depth, v, at, False)
    assert gv[0] == -3.0 and ga[0] == 77 and gv[1] == -3.0 and np.signbit(gv[3]) and ga[3] == 12
