"""What test_gpu_lwa_fast.py stands on, pinned without a GPU: the exact-sum planes of lwa_fast_cases (the model of the interval
kernel's chain equals the oracle bit for bit on them; the model's single-step defects are noticed) and lwa_plan_ref.fast_plan (a
hand-worked table of the CG ladder, the virtual blocks and the column groups a persistent workgroup visits)."""
import numpy as np
import pytest

import xcontour_oracle as O
import lwa_fast_cases as C
import lwa_plan_ref as P


def _oracle(case, name):
    return O.cal_local_wave_activity(case['q'].astype(np.float64), case['Q'], case['coord'], case['dA'], case['increase'], name,
                                     metric=case['M'])


# ---------------------------------------------------------------- 1. the cases and the model
def test_builder_gives_what_it_promises():
    """a 'mixed' state holds integers and half-integers, a long plateau and one at each end, and reaches past the tracer on both sides;
    cells tie with levels; NaN cells, a NaN column, NaN weights, a weight of exactly 256; both sides of the sum are non-zero"""
    for ny, inc in ((600, True), (1905, False), (67, True)):
        c = C.build(ny, 9, 'f32' if ny == 67 else 'f64', inc, seed=ny)
        f = C.facts(c)
        assert f['integers'] and f['halves'] and f['past_low'] and f['past_high'] and f['ties'] > 0
        assert f['longest'] >= (70 if ny >= 280 else ny // 4) and f['first_run'] >= 2 and f['last_run'] >= 2
        assert c['qnan'].all(axis=0).sum() == 1 and c['qnan'].sum() > ny and c['dAnan'].sum() >= 1 and c['Mnan'].sum() >= 1
        assert (c['dAi'] == 256).any() and c['dAi'].min() >= 1 and c['Mi'].min() >= 1 and c['Mi'].max() <= 16
        d = np.diff(c['Q'])
        assert (d >= 0).all() if inc else (d <= 0).all()
        if ny == 67:
            up, lo = _oracle(c, 'upper'), _oracle(c, 'lower')
            assert (up != 0).any() and (lo != 0).any()
    C.check_bound(5716, 2 ** 21, 256 * 256)                        # the largest plane with the widest state: 2^12.5 * 2^22 * 2^16
    with pytest.raises(AssertionError):                            # a case that breaks exactness cannot be written
        C.check_bound(5716, 2 ** 24, 256 * 256)


def test_planted_columns_hold_their_property():
    for inc in (True, False):
        c = C.build(80, 6, increase=inc, planted=((0, 'below'), (1, 'above'), (3, 'desc'), (5, 'plateau')), seed=3)
        s = 1 if inc else -1
        qp, Qp = s * c['q2'], s * c['Q2']
        assert not c['qnan'][:, [0, 1, 3, 5]].any()
        assert (qp[:, 0] < Qp[0]).all() and (qp[:, 1] > Qp[-1]).all() and (np.diff(qp[:, 3]) < 0).all()
        assert (qp[:, 5] == qp[0, 5]).all() and (Qp == qp[0, 5]).sum() == C.plateau_len(80)
        for name, pc in C.PARTS:
            ref = _oracle(c, name)
            assert np.array_equal(C.model(c, pc), ref)
            if name != 'all':                                      # one-sided columns: the near side of 'below', the far side of 'above'
                near = (name == 'upper') == inc
                assert (ref[:, 0] != 0).any() == near and (ref[:, 1] != 0).any() == (not near)


@pytest.mark.parametrize('increase', [True, False])
@pytest.mark.parametrize('dt', ['f64', 'f32'])
def test_model_equals_the_oracle_bit_for_bit(dt, increase):
    """both directions of the tracer and of the coordinate, every part, the six rank pairs, at 67 rows (two waves of pieces: per = 1,
    rows 64..66 behind the second half's base) -- and the special reference states, the planted columns and the scaled cases"""
    for coord_up in (True, False):
        for da, m in C.RANKS:
            c = C.build(67, 5, dt, increase, coord_up, da, m, seed=11)
            for name, pc in C.PARTS:
                assert np.array_equal(C.model(c, pc), _oracle(c, name)), (coord_up, da, m, name)
    extra = [dict(state=st, seed=12) for st in C.STATES[1:]] + [dict(planted=((0, 'desc'), (1, 'plateau'), (3, 'below'), (4, 'above')), seed=13)]
    if dt == 'f64':
        extra += [dict(k=500, seed=14), dict(k=-500, seed=14)]
    for kw in extra:
        c = C.build(40, 5, dt, increase, da='plane', m=None, **kw)
        for name, pc in C.PARTS:
            ref = _oracle(c, name)
            assert np.isfinite(ref).all() and np.array_equal(C.model(c, pc), ref), (kw, name)
    for ny in (2, 3, 129, 257):                                    # the smallest plane; per = 2 and 3
        c = C.build(ny, 2, dt, increase, da='row', m='plane', seed=15)
        assert np.array_equal(C.model(c, 0), _oracle(c, 'all')), ny


def test_sampled_rows_are_the_oracles_rows():
    """lwa_rows (the oracle's loop body for chosen target rows) against the oracle's planes, and the rows sample_rows picks"""
    for inc in (True, False):
        for da, m in C.RANKS:
            c = C.build(131, 7, 'f32', inc, not inc, da, m, seed=21)
            rows = C.sample_rows(131)
            for name, _ in C.PARTS:
                got = C.lwa_rows(c['q'], c['Q'], c['coord'], c['dA'], rows, inc, name, c['M'])
                assert np.array_equal(got, _oracle(c, name)[rows])
    # per = ceil(1905 / 128) = 15: piece edges 15, 960, 975
    assert C.sample_rows(1905) == [0, 1, 2, 13, 14, 15, 16, 951, 952, 953, 958, 959, 960, 961, 973, 974, 975, 976, 1902, 1903, 1904]
    assert C.sample_rows(2) == [0, 1] and C.sample_rows(64) == [0, 1, 2, 31, 32, 33, 61, 62, 63]
    assert 20 <= len(C.sample_rows(5716)) <= 24


# the cases of the defect table: (name, build keywords, part)
DEFECT_CASES = [
    ('row dA, no M', dict(ny=24, nx=4, da='row', m=None, seed=4), 0),
    ('130 rows', dict(ny=130, nx=3, da='plane', m=None, seed=5), 0),
    ('decreasing, upper', dict(ny=24, nx=4, increase=False, da='plane', m='row', seed=2), 1),
]
# Three of the eight single-step defects cannot change ANY result, in exact arithmetic or in the kernel's doubles on exact planes:
#   * 'a_for_b' / 'b_for_a' (one bound of the search used for the other): the two differ only for a cell that ties with levels, and
#     they move the interval's end only across targets j with Q'_j = q'_y -- whose term (Q'_j - q'_y) W is zero on either side;
#   * 'b_ge_y1' (b >= y + 1 for b >= y + 2): the extra case b = y + 1 adds +W and -W to the SAME index y + 1.
# They are rounding-only rewrites of the kernel; the test holds them to "no change on any case" so that the argument stays checked.
NEUTRAL = ('a_for_b', 'b_for_a', 'b_ge_y1')


def test_every_defect_is_noticed_and_every_case_is_needed():
    built = [(name, C.build(**kw), part) for name, kw, part in DEFECT_CASES]
    base = [C.model_int(c, part) for _, c, part in built]
    for (name, c, part), b in zip(built, base):
        pname = C.PARTS[part][0]
        assert np.array_equal(C.model(c, part), _oracle(c, pname)), name
    caught = {d: [name for (name, c, part), b in zip(built, base) if C.model_int(c, part, d) != b] for d in C.DEFECTS}
    for d in C.DEFECTS:
        assert bool(caught[d]) == (d not in NEUTRAL), (d, caught[d])
    # every case is the ONLY one to notice some defect: without it that defect would pass
    assert caught['m_rank'] == ['row dA, no M'] and caught['no_half_base'] == ['130 rows'] and caught['side'] == ['decreasing, upper']
    assert len(caught['a_lt_y']) >= 1 and len(caught['minus_at_y']) == len(DEFECT_CASES)


def test_neutral_defects_change_nothing_anywhere():
    """the three rewrites above on cases crowded with ties (constant and two-level states, a column on the plateau), every part"""
    for kw in (dict(state='constant'), dict(state='two'), dict(), dict(increase=False)):
        c = C.build(70, 4, seed=31, planted=((1, 'plateau'), (2, 'desc')), **kw)
        assert C.facts(c)['ties'] >= 70
        for _, pc in C.PARTS:
            b = C.model_int(c, pc)
            for d in NEUTRAL:
                assert C.model_int(c, pc, d) == b, (kw, pc, d)


# ---------------------------------------------------------------- 2. the interval plan, by hand
# lwa_fast_lds: (1 + 2 CG)(ny + 1) doubles + 4097 ints = 8 (1 + 2 CG)(ny + 1) + 16388 bytes against kLdsBudget = 153600:
#   CG 4: 72 (ny + 1) <= 137212 -> ny <= 1904      CG 2: 40 (ny + 1) -> ny <= 3429      CG 1: 24 (ny + 1) -> ny <= 5716
RUNGS = [
    (1904, 4, 72 * 1905 + 16388),      # 153548: 52 bytes to spare
    (1905, 2, 40 * 1906 + 16388),      # CG 4 would be 153620;  92628
    (3429, 2, 40 * 3430 + 16388),      # 153588: 12 bytes to spare
    (3430, 1, 24 * 3431 + 16388),      # CG 2 would be 153628;  98732
    (5716, 1, 24 * 5717 + 16388),      # 153596: the bucket table ends 4 bytes under the budget
    (5717, None, 24 * 5718 + 16388),   # 153620: no interval kernel
]


@pytest.mark.parametrize('ny,CG,nbytes', RUNGS)
def test_fast_plan_rung_edges(ny, CG, nbytes):
    p = P.fast_plan(1, ny, 9)
    if CG is None:
        assert p is None and P.fast_lds_bytes(ny, 1) == nbytes > P.LDS_BUDGET == 153600
    else:
        assert (p['CG'], p['lds_bytes']) == (CG, nbytes) and nbytes <= 153600
        assert CG == 4 or P.fast_lds_bytes(ny, 2 * CG) > 153600
    assert [RUNGS[i][2] for i in (0, 2, 4)] == [153548, 153588, 153596]


def test_fast_plan_virtual_blocks_and_grid():
    """CG 4: 4 groups per 16-column line, 8 XCDs: nvb is the group count padded to 32; one workgroup per CU, a multiple of 8"""
    for nx, ngrp, nvb in ((1, 1, 32), (128, 32, 32), (129, 33, 64), (3600, 900, 928)):
        p = P.fast_plan(3, 70, nx)
        assert (p['CG'], p['nvb'], p['grid']) == (4, nvb, (min(nvb, 256), 3)) and -(-nx // 4) == ngrp
    assert P.fast_plan(1, 70, 3600, cus=0)['grid'] == (256, 1) and P.fast_plan(1, 70, 3600, cus=304)['grid'] == (304, 1)
    assert P.fast_plan(1, 70, 3600, cus=100)['grid'] == (96, 1) and P.fast_plan(1, 70, 3600, cus=5)['grid'] == (8, 1)
    assert P.fast_plan(1, 1905, 129)['nvb'] == 128 and P.fast_plan(1, 3430, 129)['nvb'] == 256       # CG 2: pads to 64, CG 1: to 128
    assert P.fast_plan(1, 600, (1 << 29) // 600 + 1) is None and P.fast_plan(1, 600, (1 << 29) // 600) is not None    # 32-bit offsets


def test_fast_plan_visit_lists_by_hand():
    """vb = 8 kq + xcd -> column ((kq // GQ) * 8 + xcd) * 16 + (kq % GQ) * CG, GQ = 16 / CG; a block walks vb, vb + grid, ...
    CG 4 (GQ 4), 70 x 3600 on 256 CUs: nvb 928, so trips at kq = b / 8, + 32, + 64, + 96: lines + 64 each = columns + 1024.
    The plane has 225 lines of 16 columns: of the last 8 kq (112..115 -> lines 224 + xcd) only xcd 0 is inside."""
    p = P.fast_plan(1, 70, 3600)
    v, sk = p['visits'], p['skips']
    assert v[0] == [(0, 4), (1024, 4), (2048, 4), (3072, 4)]
    assert v[7] == [(112, 4), (1136, 4), (2160, 4), (3184, 4)]              # xcd 7: line 7
    assert v[8] == [(4, 4), (1028, 4), (2052, 4), (3076, 4)]                # kq 1: the second group of line 0
    assert v[255] == [(1020, 4), (2044, 4), (3068, 4)]                      # kq 31, xcd 7: line 63, group 3; vb 1023 is past nvb
    assert v[129] == [(528, 4), (1552, 4), (2576, 4)] and sk[129] == [('mid', 3)]      # vb 897: kq 112, xcd 1 -> line 225: outside
    assert v[128] == [(512, 4), (1536, 4), (2560, 4), (3584, 4)] and sk[128] == []     # vb 896: xcd 0 -> line 224: the last one
    # CG 1 (GQ 16), 3430 x 300: nvb 384 (300 groups padded to 128), trips at kq and kq + 32: lines + 16 = columns + 256
    p = P.fast_plan(1, 3430, 300)
    v, sk = p['visits'], p['skips']
    assert (p['CG'], p['nvb'], p['grid']) == (1, 384, (256, 1))
    assert v[0] == [(0, 1), (256, 1)] and v[8] == [(1, 1), (257, 1)]
    assert v[7] == [(112, 1)] and sk[7] == [('mid', 1)]                      # vb 263: line 16 + 7 = column 368: outside
    assert v[255] == [(255, 1)] and sk[255] == []                           # kq 31, xcd 7: line 15, column 15; vb 511 is past nvb
    # a plane narrower than the padding: the surplus blocks find nothing on entry
    p = P.fast_plan(1, 70, 5)
    assert p['grid'] == (32, 1) and p['visits'][0] == [(0, 4)] and p['visits'][8] == [(4, 1)]
    assert all(p['visits'][b] == [] and p['skips'][b] == [('entry', 0)] for b in range(32) if b not in (0, 8))


def gpu_shapes(cus):
    """every (ny, nx) the GPU suite runs on the interval kernel, the CU-dependent ones for `cus`"""
    import test_gpu_lwa_fast as T
    return T.shapes(cus)


@pytest.mark.parametrize('cus', [256, 304, 64])
def test_fast_plan_visits_cover_every_column_once(cus):
    for ny, nx in gpu_shapes(cus):
        p = P.fast_plan(1, ny, nx, cus)
        if p is None:
            assert ny > 5716
            continue
        cols = sorted(x for v in p['visits'] for x0, n in v for x in range(x0, x0 + n))
        assert cols == list(range(nx)), (ny, nx)
        assert all(x0 % p['CG'] == 0 and 1 <= n <= p['CG'] for v in p['visits'] for x0, n in v)
        assert p['grid'][0] % 8 == 0 and p['nvb'] % p['grid'][0] % 8 == 0


def test_one_round_of_loads_and_two_waves_per_array_on_every_rung():
    """for every ny a rung admits, a group's ny * CG cells fit ONE round of 8 cells x 1024 threads and four prefix tasks per column fit
    the 16 waves: the kernel's further-rounds branch (`i0 != tid`, loads that are not prefetched) and the `split == 1` arm of its
    prefix sums cannot be reached with a 1024-thread launch and a 150 KB budget.  A change of budget or block size that makes them
    reachable fails here and asks for pins of its own."""
    assert P.LDS_BUDGET == 150 * 1024 and P.FAST_THREADS == 1024 and P.FAST_CPT == 8
    edge = {4: 1904, 2: 3429, 1: 5716}
    for ny in range(2, 5800):
        p = P.fast_plan(1, ny, 16)
        if p is None:
            assert ny > 5716
            continue
        CG = p['CG']
        assert ny <= edge[CG] and (CG == 4 or ny > edge[2 * CG])
        ncell, rounds, split = P.fast_rounds(ny, CG)
        assert ncell == ny << {4: 2, 2: 1, 1: 0}[CG] <= 8 * 1024 and rounds == 1
        assert 4 * CG <= 16 and split == 2
    assert P.fast_rounds(1904, 4)[0] == 7616 and P.fast_rounds(3429, 2)[0] == 6858
