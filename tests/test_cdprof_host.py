"""cdprof_ref, the numpy restatement of K28 (composites by distance), on a hand case whose distances are exact, against two
deliberately wrong bin rules on that very case; and the host layer of Context.contour_distance_profile and the facade's refusals over a
stand-in library.  No GPU here."""
import ctypes as C

import numpy as np
import pytest

import cdprof_ref as PR
import cdprof_standin as ST
import contour_join_ref as JR
import xcontour_amd as xa
from xcontour_amd import _native as nat

# ------------------------------------------------------------------ the hand case: q[y, x] = y on integer coordinates, level 2.5
HNY, HNX = 8, 6
HQ = np.repeat(np.arange(HNY, dtype=np.float64)[:, None], HNX, axis=1)
HY, HX = np.arange(HNY, dtype=np.float64), np.arange(HNX, dtype=np.float64)


def hand(edges, signed=False, rule='histogram', w=None, fields=()):
    rec = JR.stack_records(HQ[None], np.array([2.5]))
    return PR.reference(rec, HNY, HNX, False, 0, HY, HX, edges, 1, w=w, fields=fields, signed=signed, rule=rule)


def test_the_hand_case_has_exact_distances():
    rec = JR.stack_records(HQ[None], np.array([2.5]))
    d = PR.distances(rec, HNY, HNX, False, 0, HY, HX)
    assert np.array_equal(d[0], np.repeat(np.abs(HY - 2.5)[:, None], HNX, axis=1))
    s = PR.distances(rec, HNY, HNX, False, 0, HY, HX, signed=True)
    assert np.array_equal(s[0], np.repeat((2.5 - HY)[:, None], HNX, axis=1))        # negative on the side of the larger rows


def test_the_bin_rule_on_the_hand_case():
    """edges 0.5, 1.5, 2.5: rows 2 and 3 (d = 0.5, ON the first edge) fall in bin 0; rows 1 and 4 (1.5, on the inner edge) in bin 1;
    rows 0 and 5 (2.5, the closed last edge) in bin 1; rows 6 and 7 nowhere"""
    ref = hand([0.5, 1.5, 2.5])
    assert ref['nodes'].tolist() == [[12, 24]] and ref['area'].tolist() == [[12.0, 24.0]]
    sg = hand([-2.5, -0.5, 0.5, 2.5], signed=True)
    assert sg['nodes'].tolist() == [[12, 6, 18]]            # rows 5, 4 | row 3 | rows 2, 1, 0 (the last edge closed)


@pytest.mark.parametrize('rule', [r for r in PR.RULES if r != 'histogram'])
def test_a_wrong_bin_rule_gives_other_counts_on_the_hand_case(rule):
    assert hand([0.5, 1.5, 2.5], rule=rule)['nodes'].tolist() == [[12, 12]]
    assert hand([-2.5, -0.5, 0.5, 2.5], signed=True, rule=rule)['nodes'].tolist() != [[12, 6, 18]]


def test_sums_skip_nan_flag_inf_and_widen_float32():
    w = np.repeat((1.0 + 0.25 * HY)[:, None], HNX, axis=1)
    f = (HQ * 0.1).astype(np.float32)
    g = HQ.copy(); g[2, 1] = np.nan; g[4, 0] = np.inf
    ref = hand([0.5, 1.5, 2.5], w=w, fields=[f, g])
    assert ref['area'][0, 0] == 6 * (w[2, 0] + w[3, 0])
    import math
    assert ref['sums'][0, 0, 0] == math.fsum((w[2:4] * f[2:4].astype(np.float64)).ravel().tolist())
    assert ref['sums'][1, 0, 0] == math.fsum(np.delete((w[2:4] * HQ[2:4]).ravel(), 1).tolist())      # the NaN node skipped
    assert np.isnan(ref['sums'][1, 0, 1]) and ref['nodes'].tolist() == [[12, 24]]


# ------------------------------------------------------------------ the host layer over a stand-in library
S, NY, NX = 2, 6, 8
LV = np.array([-0.5, 0.0, 0.5])
Y, X = np.arange(NY, dtype=np.float64), np.arange(NX, dtype=np.float64)
EDGES = [0, 1, 2, 4]                                                            # (integers: the binding hands float64 to the library)
K12, K28 = ST.ST.SL._K12, ST.K28


@pytest.fixture
def sctx():
    c = nat.Context.__new__(nat.Context)
    c.lib, c.handle, c.device = ST.Lib(), None, 0
    c._buffers, c._resident, c._staged, c._ev_pool = [], {}, [], []
    c.max_batch_bytes = 8 << 30
    return c


def _segments(lib, a):
    """a scripted K12: two segments in every range"""
    if a[9]:
        return 0
    lib.poke(a[10], np.full(a[3] * a[7], 2, dtype=np.uint64))
    return 1


def _host(v, ctype, n):
    at = v.value if isinstance(v, C.c_void_p) else v
    return list((ctype * n).from_address(at))


def test_argument_order_edges_fields_and_the_mask_of_k17(sctx):
    got = {}

    def k28(lib, a):                                                            # host arrays are read while the call is live
        got['edges'] = _host(a[17], C.c_double, a[16])
        got['f'], got['dt'], got['ps'] = _host(a[22], C.c_void_p, a[21]), _host(a[23], C.c_int, a[21]), _host(a[24], C.c_int, a[21])
        return 0
    sctx.lib.on.update({k: _segments for k in K12})
    sctx.lib.on[K28] = k28
    q = np.zeros((S, NY, NX))
    w = np.ones((NY, NX))
    f0, f1 = np.ones((NY, NX), dtype=np.float32), np.ones((S, NY, NX))
    nodes, area, sums, flags = sctx.contour_distance_profile(q, LV, Y, X, EDGES, w=w, fields=[f0, f1], period=NX + 1.0, select='main',
                                                             max_distance=4.0, signed=True, flip=True)
    assert nodes.shape == area.shape == (S, 3, 3) and nodes.dtype == np.int64 and area.dtype == np.float64
    assert sums.shape == (S, 3, 2, 3) and flags.shape == (S, 3, 3) and flags.dtype == np.int32
    assert [c[0] for c in sctx.lib.calls] == list(K12[1:]) * 2 + ['xc_contour_interior_dev', K28]
    k17, a = sctx.lib.args[2][1], sctx.lib.args[3][1]
    assert len(a) == len(nat.PROTOTYPES[K28][1])
    assert a[1] == k17[1] == S * 3 and a[2:6] == k17[2:6] and a[6:10] == (NY, NX, 1, 2) and a[12:15] == (NX + 1.0, 0.0, 4.0)
    assert k17[10:12] == (1, 3)                                                 # flip, ncont
    assert a[15] == k17[19] and sctx.lib.where(a[15])[1] == S * 3 * NY * NX     # negate_mask IS K17's mask
    assert a[16] == 4 and got['edges'] == [0.0, 1.0, 2.0, 4.0] and not isinstance(sctx.lib.where(a[17]), tuple)   # (a host array)
    assert a[18] == 3 and sctx.lib.where(a[19])[1] == NY * NX * 8 and a[20] == 0 and a[21] == 2
    assert [sctx.lib.where(v)[1] for v in got['f']] == [NY * NX * 4, S * NY * NX * 8]
    assert got['dt'] == [nat.XC_F32, nat.XC_F64] and got['ps'] == [0, 1]
    assert [sctx.lib.where(v)[1] for v in a[25:29]] == [S * 3 * 3 * 8, S * 3 * 3 * 8, 2 * S * 3 * 3 * 8, S * 3 * 3 * 4]


def test_without_fields_weights_or_sign(sctx):
    sctx.lib.on.update({k: _segments for k in K12})
    nodes, area, sums, flags = sctx.contour_distance_profile(np.zeros((S, NY, NX)), LV, Y, X, EDGES)
    assert sums.shape == (S, 3, 0, 3) and flags.shape == (S, 3, 1)
    a = sctx.lib.args[-1][1]
    assert [c[0] for c in sctx.lib.calls] == list(K12[:1]) * 2 + [K28]
    assert a[15] is None and a[19] is None and a[20:22] == (0, 0) and a[27] is None and a[12:15] == (0.0, 0.0, 0.0)


def test_contours_go_in_groups_under_the_mask_only_when_signed(sctx):
    sctx.lib.on.update({k: _segments for k in K12})
    sctx.max_batch_bytes = NY * NX * 2                                          # two mask planes: one slab of two contours per call
    res = sctx.contour_distance_profile(np.zeros((S, NY, NX)), LV, Y, X, EDGES, fields=[np.ones((NY, NX))], signed=True)
    assert [v.shape for v in res] == [(S, 3, 3), (S, 3, 3), (S, 3, 1, 3), (S, 3, 2)]
    assert sorted(n for k, n in sctx.lib.calls if k == K28) == [1, 1, 2, 2]
    assert [a[1][18] for a in sctx.lib.args if a[0] == K28] == [2, 2, 1, 1]     # ncont is the group's
    sctx.lib.calls[:] = []
    sctx.contour_distance_profile(np.zeros((S, NY, NX)), LV, Y, X, EDGES)      # no plane per contour on the device: all contours at once
    assert [n for k, n in sctx.lib.calls if k == K28] == [3, 3]


@pytest.mark.parametrize('kw,text', [
    (dict(edges=[0.0, 2.0, 2.0]), 'edges must be 2 to 4097 finite, strictly ascending'),
    (dict(edges=[0.0, 2.0, 1.0]), 'edges must be 2 to 4097 finite, strictly ascending'),
    (dict(edges=[0.0, np.nan]), 'edges must be 2 to 4097 finite, strictly ascending'),
    (dict(edges=[0.0, np.inf]), 'edges must be 2 to 4097 finite, strictly ascending'),
    (dict(edges=[1.0]), 'edges must be 2 to 4097 finite, strictly ascending'),
    (dict(edges=np.arange(4098.0)), 'edges must be 2 to 4097 finite, strictly ascending'),
    (dict(fields=[np.ones((NY, NX))] * 9), 'at most 8 fields'),
    (dict(select='main'), 'needs periodic=True'),
    (dict(w=np.ones(NY)), 'w must be'),
    (dict(max_distance=float('nan')), 'max_distance is NaN'),
])
def test_refusals_of_the_binding_reach_no_kernel(sctx, kw, text):
    args = dict(edges=EDGES)
    args.update(kw)
    with pytest.raises(nat.XContourHipError, match=text) as e:
        sctx.contour_distance_profile(np.zeros((S, NY, NX)), LV, Y, X, args.pop('edges'), **args)
    assert 'xc_contour_distance_profile' in str(e.value) and sctx.lib.calls == []


def test_the_facade_refuses_before_it_opens_a_device():
    q = xa.DataArray(HQ, ('y', 'x'), {'y': HY, 'x': HX}, 'q')
    cm = xa.Contour2D(q, np.ones(HNY), {'X': 'x', 'Y': 'y'}, {'Y': 'y'}, dtype=np.float64)
    lv = xa.DataArray(np.array([2.5]), ('contour',), {'contour': np.arange(1)}, 'q')
    with pytest.raises(Exception, match='needs periodic'):
        cm.cal_contour_distance_profile(lv, [0.0, 1.0], select='main')
    with pytest.raises(Exception, match='bins should be at least two finite, ascending edges'):
        cm.cal_contour_distance_profile(lv, [0.0, 1.0, 1.0])
    with pytest.raises(Exception, match='bins should be at least two finite, ascending edges'):
        cm.cal_contour_distance_profile(lv, [0.0, np.nan])
    assert callable(xa.distance_profile)
