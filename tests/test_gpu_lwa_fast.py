"""-m gpu: K7F, the interval kernel (k_lwa_fast), bit for bit on planes whose sums are exact.

Every field comes from lwa_fast_cases.build: integer and half-integer cells and levels, integer weights with max 256 = 2^8 -- every term,
every partial sum in any order, the kernel's difference arrays, prefix sums and its final difference of two products are exact doubles
(the builder asserts the bound with Python integers).  So the oracle's literal loop (core.py:752-791), the band walk (`exact=True`) and
the interval kernel must return the SAME bits: every comparison here is np.array_equal, and a mismatch is a wrong term -- a wrong prefix
base, a group stored to the wrong columns, a stale register of the prefetched round -- never rounding.

The calls go through ctx.lwa(..., exact=False): the premises are checked on the host and the interval kernel runs for ANY plane height
(one launch); ctx.last_lwa_path() is asserted after every call.  What a shape makes the kernel do -- columns per workgroup (CG), trips of
the persistent loop, surplus groups skipped, a ragged last group -- cannot be seen from outside: it is lwa_plan_ref.fast_plan's, pinned on
a hand-worked table by test_lwa_fast_host.py, and each test asserts on the plan what it means to reach before the GPU is asked.

References: small planes the oracle on every row; tall planes the oracle's loop body on lwa_fast_cases.sample_rows (the first and last
rows, the rows around the level c = Q'[ny / 2], both sides of the edges of the prefix-sum pieces) AND every row of the band walk, which
test_gpu_lwa_walk.py pins on the oracle.
"""
import numpy as np
import pytest

import xcontour_oracle as O
import lwa_fast_cases as C
import lwa_plan_ref as P

pytestmark = pytest.mark.gpu

B_NY = (2, 63, 64, 65, 127, 128, 129, 255, 257, 513, 640)        # around the piece edges of the prefix sums: per = 1 | 2 | 3 | 5
C_NX = (1, 2, 3, 4, 5, 126, 127, 128, 129, 131)                  # groups and ragged ends at CG 4
E_NY = (1904, 1905, 3429, 3430, 5716)                            # the tightest LDS fit of every rung and the first row count of the next
D_NY = {4: 70, 2: 1905, 1: 3430}


def d_nx(CG, cus):
    """section D: a plane of D_NY[CG] rows with more than two groups per workgroup of the grid, whose plan has blocks with three visits
    and blocks with two, a surplus group skipped in mid-loop, and (CG > 1) a ragged last group visited as a second or later trip"""
    ny = D_NY[CG]
    grid = P.fast_plan(1, ny, 1 << 14, cus)['grid'][0]                  # a plane wide enough to fill the chip: one workgroup per CU
    gq = 8 * (16 // CG)
    first = 2 * grid + 1 + min(gq + gq // 2, grid // 2)                 # a line and a half into the third trip
    for ngrp in list(range(first, 3 * grid + 1)) + list(range(2 * grid + 1, first)):
        nx = ngrp * CG - (1 if CG > 1 else 0)
        if d_reaches(P.fast_plan(1, ny, nx, cus), CG):
            return nx
    raise AssertionError((CG, cus))


def d_reaches(p, CG):
    trips = [len(v) for v in p['visits']]
    ragged = [i for v in p['visits'] for i, (x0, n) in enumerate(v) if n < CG]
    return (p['CG'] == CG and max(trips) == 3 and min(trips) == 2 and any(k == 'mid' for sk in p['skips'] for k, _ in sk)
            and (CG == 1 or (len(ragged) == 1 and ragged[0] >= 1)))


def shapes(cus):
    """every (ny, nx) this module runs on the interval kernel (test_lwa_fast_host.py: the visit lists cover each exactly once)"""
    return ([(67, 37)] + [(ny, 9) for ny in B_NY] + [(70, nx) for nx in C_NX] + [(D_NY[CG], d_nx(CG, cus)) for CG in (4, 2, 1)]
            + [(ny, 9) for ny in E_NY] + [(600, 13), (70, 9), (1905, 7)])


def _lwa(ctx, c, pc, exact=False, path=1):
    out, _ = ctx.lwa(c['q'][None], c['Q'][None], c['coord'], c['dA'], c['dA_max'], M=c['M'], increase=c['increase'], part=pc, exact=exact)
    assert ctx.last_lwa_path() == path, (ctx.last_lwa_path(), path)
    return out[0]


def _oracle(c, name):
    return O.cal_local_wave_activity(c['q'].astype(np.float64), c['Q'], c['coord'], c['dA'], c['increase'], name, metric=c['M'])


def _same(got, ref, what, rows=None):
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        j = bad[0][0] if rows is None else rows[bad[0][0]]
        raise AssertionError('%r: %d cells differ, first at target row %d column %d: %r != %r (reference)'
                             % (what, len(bad), j, bad[0][1], got[tuple(bad[0])], ref[tuple(bad[0])]))


def _tall(ctx, c, parts=C.PARTS, path=1):
    """a tall plane: the interval kernel against the oracle's loop body on the sampled rows and against every row of the band walk"""
    rows = C.sample_rows(c['ny'])
    for name, pc in parts:
        got = _lwa(ctx, c, pc, path=path)
        assert np.isfinite(got).all()
        ref = C.lwa_rows(c['q'], c['Q'], c['coord'], c['dA'], rows, c['increase'], name, c['M'])
        assert (ref != 0).any()
        _same(got[rows], ref, (c['ny'], c['nx'], c['dt'], name, 'sampled rows'), rows)
        _same(got, _lwa(ctx, c, pc, exact=True, path=0), (c['ny'], c['nx'], c['dt'], name, 'band walk'))


# ---------------------------------------------------------------- A. every mode
@pytest.mark.parametrize('increase', [True, False], ids=['inc', 'dec'])
@pytest.mark.parametrize('dt', ['f64', 'f32'])
def test_every_mode_at_67_rows(ctx, dt, increase):
    """67 x 37 (ten groups, the last with one column; rows 64..66 behind the second half's prefix base): both tracer types and
    directions x both coordinate directions x every part x the six rank pairs of weight and metric = 144 calls, each against the oracle.
    Catches: `side` swapped, a weight or metric indexed by the wrong rank (dA by row WITH an M; no M falling back to dA's rank)."""
    p = P.fast_plan(1, 67, 37, ctx.device_cus())
    assert p['CG'] == 4 and sum(len(v) for v in p['visits']) == 10 and (36, 1) in [g for v in p['visits'] for g in v]
    for coord_up in (True, False):
        for da, m in C.RANKS:
            c = C.build(67, 37, dt, increase, coord_up, da, m, seed=101)
            for name, pc in C.PARTS:
                _same(_lwa(ctx, c, pc), _oracle(c, name), (dt, increase, coord_up, da, m, name))


# ---------------------------------------------------------------- B. the pieces of the prefix sums
@pytest.mark.parametrize('ny', B_NY)
def test_prefix_sum_pieces(ctx, ny):
    """128 pieces of per = ceil(ny / 128) rows, the second wave of an array starting from the first one's total: row counts on both
    sides of 64 per and of a whole number of pieces -- empty pieces (ny = 2: 126 of them), a second half that is empty (64), holds one
    row (65) or is full (128), per = 2 with one row in the last live piece (129), per = 3, 5.  2 is the smallest plane the entry point
    takes.  513 and 640 also through the gated default mode (planes of more than 512 rows).
    Catches: a wrong or missing base of the second half, a piece that reads past ny, an off-by-one at p = 0, p = ny or y + 1 = ny."""
    p = P.fast_plan(1, ny, 9, ctx.device_cus())
    assert p['CG'] == 4 and p['visits'][0] == [(0, 4)] and p['visits'][8] == [(4, 4)] and p['visits'][16] == [(8, 1)]
    for increase, dt, da, m in ((True, 'f64', 'plane', 'row'), (False, 'f32', 'row', None)):
        c = C.build(ny, 9, dt, increase, True, da, m, seed=200 + ny, planted=((0, 'desc'), (8, 'above')))
        for name, pc in C.PARTS:
            ref = _oracle(c, name)
            _same(_lwa(ctx, c, pc), ref, (ny, increase, name))
            if ny > 512:
                _same(_lwa(ctx, c, pc, exact=None), ref, (ny, increase, name, 'gated'))


# ---------------------------------------------------------------- C. groups and ragged ends
@pytest.mark.parametrize('nx', C_NX)
def test_groups_and_ragged_ends_at_four_columns(ctx, nx):
    """70 rows, planes of less than one group to 33 groups: ncol = 1, 2, 3 in the last group, one group only, exactly 32 groups (one
    XCD round: nvb = 32, no surplus) and 33 (nvb = 64: 31 surplus blocks that find nothing on entry).
    Catches: columns >= ncol of a ragged group read or stored, a group stored at another group's columns, a surplus block that runs."""
    p = P.fast_plan(1, 70, nx, ctx.device_cus())
    groups = sorted(g for v in p['visits'] for g in v)
    assert p['CG'] == 4 and len(groups) == -(-nx // 4) and groups[-1][1] == (nx - 1) % 4 + 1
    assert p['nvb'] == (64 if nx > 128 else 32) and all(len(v) <= 1 for v in p['visits'])
    assert sum(1 for sk in p['skips'] if sk == [('entry', 0)]) == p['nvb'] - len(groups)
    for increase, da, m, dt in ((True, 'plane', 'plane', 'f64'), (False, 'row', 'row', 'f32')):
        c = C.build(70, nx, dt, increase, True, da, m, seed=300 + nx)
        for name, pc in C.PARTS[:2] if increase else C.PARTS[::2]:
            _same(_lwa(ctx, c, pc), _oracle(c, name), (nx, increase, name))


# ---------------------------------------------------------------- D. second and third trips of the persistent loop
@pytest.mark.parametrize('CG', [4, 2, 1])
def test_second_and_third_trips(ctx, CG):
    """one plane per rung wide enough that workgroups run the loop body three times: the next group's cells are requested under this
    group's prefix sums, surplus groups are stepped over in mid-loop, and (CG 4, CG 2) the ragged last group arrives as a prefetched
    third trip.  With a grid that is a whole number of XCD rounds (256 CUs) a trip either exists for every block of a line or for none
    before it, so blocks with 1, 2 AND 3 visits cannot share one plan: this plane has 2 and 3 (blocks with one visit: sections B, C, E).
    Catches: a register of the prefetched round used for the wrong group, D0 / D1 not cleared between groups, a skipped group's loads
    consumed, the ragged group's columns taken from the group before."""
    cus = ctx.device_cus()
    ny, nx = D_NY[CG], d_nx(CG, cus)
    p = P.fast_plan(1, ny, nx, cus)
    assert d_reaches(p, CG) and p['nvb'] > 2 * p['grid'][0]
    trips = [len(v) for v in p['visits']]
    print('D: CG %d on %d CUs: %d x %d, nvb %d, grid %d, blocks with 2 / 3 visits: %d / %d, mid-loop skips %d'
          % (CG, cus, ny, nx, p['nvb'], p['grid'][0], trips.count(2), trips.count(3), sum(len(sk) for sk in p['skips'])))
    c = C.build(ny, nx, 'f64', True, True, 'plane', 'row', seed=400 + CG)
    if CG == 4:
        for name, pc in C.PARTS:
            _same(_lwa(ctx, c, pc), _oracle(c, name), (CG, nx, name))
    else:
        _tall(ctx, c, parts=C.PARTS[:1])


# ---------------------------------------------------------------- E. the tightest LDS fit of every rung
@pytest.mark.parametrize('dt', ['f64', 'f32'])
@pytest.mark.parametrize('ny', E_NY)
def test_rung_edges_and_tightest_lds_fit(ctx, ny, dt):
    """1904 | 1905, 3429 | 3430, 5716: the last row count of every rung (the bucket table ends 52, 12 and 4 bytes under the budget) and
    the first of the next; weight and metric planes (three loads per cell).
    Catches: a layout that overruns its allotment (D1's last row into the bucket table, the table past the LDS), a CG-dependent index."""
    p = P.fast_plan(1, ny, 9, ctx.device_cus())
    assert p['CG'] == {1904: 4, 1905: 2, 3429: 2, 3430: 1, 5716: 1}[ny] and p['lds_bytes'] <= P.LDS_BUDGET
    assert ny in (1905, 3430) or P.fast_plan(1, ny + 1, 9) is None or P.fast_plan(1, ny + 1, 9)['CG'] < p['CG']
    c = C.build(ny, 9, dt, ny % 2 == 0, True, 'plane', 'plane', seed=500 + ny, planted=((3, 'desc'), (4, 'plateau')))
    _tall(ctx, c, parts=C.PARTS[:1] if dt == 'f32' else C.PARTS[1:])


def test_past_the_last_rung_is_the_band_walk(ctx):
    """5717 rows: no layout fits, exact=False falls to the band walk (path 0) and the answer is the same"""
    assert P.fast_plan(1, 5717, 9, ctx.device_cus()) is None
    c = C.build(5717, 9, 'f64', True, True, 'plane', 'plane', seed=517)
    _tall(ctx, c, parts=C.PARTS[:1], path=0)


# ---------------------------------------------------------------- F. reference states
F_STATES = [dict(state='constant'), dict(state='two'), dict(state='lastbucket'), dict(k=500), dict(k=-500)]


@pytest.mark.parametrize('kw', F_STATES, ids=['constant', 'two-levels', 'last-bucket', 'scale-2^500', 'scale-2^-500'])
def test_reference_states_that_stress_the_bucket_table(ctx, kw):
    """600 x 13.  One level everywhere (bscale = 0: every cell in bucket 0, the full binary search), two levels, every level but the
    first inside the last bucket, and cells and levels scaled by 2^500 / 2^-500 (bscale ~ 2^-498 / 2^502; exact all the same).
    Catches: a bracket [G[k], G[k + 1]] that misses the lower bound, a bucket of a cell past the table, ties counted on one side."""
    for increase in (True, False):
        c = C.build(600, 13, 'f64', increase, True, 'plane', None, seed=600, **kw)
        for name, pc in C.PARTS:
            ref = _oracle(c, name)
            assert np.isfinite(ref).all() and ((ref != 0).any() or name != 'all')
            _same(_lwa(ctx, c, pc), ref, (kw, increase, name))


def test_stack_of_three_slabs_with_three_states(ctx):
    """three slabs in one launch (grid y), each with its own reference state -- mixed, two levels, last bucket -- and the third slab's
    columns reversed.  Catches: a slab reading another slab's Q' or bucket table, a slab offset on the tracer or the output."""
    cs = [C.build(600, 13, 'f64', True, True, 'plane', 'row', seed=610 + i, wseed=610, state=st) for i, st in enumerate(('mixed', 'two', 'lastbucket'))]
    q = np.stack([cs[0]['q'], cs[1]['q'], cs[2]['q'][:, ::-1]])
    Q = np.stack([c['Q'] for c in cs])
    assert all(np.array_equal(c['dA'], cs[0]['dA'], equal_nan=True) and np.array_equal(c['M'], cs[0]['M']) for c in cs)
    for name, pc in C.PARTS:
        out, _ = ctx.lwa(q, Q, cs[0]['coord'], cs[0]['dA'], 256.0, M=cs[0]['M'], increase=True, part=pc, exact=False)
        assert ctx.last_lwa_path() == 1
        for s in range(3):
            ref = O.cal_local_wave_activity(q[s], Q[s], cs[0]['coord'], cs[0]['dA'], True, name, metric=cs[0]['M'])
            _same(out[s], ref, ('slab', s, name))


# ---------------------------------------------------------------- G. planted columns
@pytest.mark.parametrize('ny,nx,xs', [(70, 9, (0, 3, 4, 8)), (1905, 7, (0, 1, 2, 6))], ids=['CG4', 'CG2'])
def test_planted_columns_at_the_group_edges(ctx, ny, nx, xs):
    """columns that are one-sided by construction -- every cell below Q'_0 (p = 0 for every cell), above Q'_last (p = ny), strictly
    descending (far-side intervals that end at y + 1 = ny), constant on the 70-level plateau (every cell ties with the whole run) -- at
    x = 0, the last column of a full group, the first of the next and the last column of the plane (a ragged group of one), each kind
    at each place; neighbours are ordinary columns.  Catches: a group's result stored one column or one group off, p at either end of
    the difference array, the upper-bound walk over a plateau."""
    p = P.fast_plan(1, ny, nx, ctx.device_cus())
    CG = p['CG']
    assert CG == (4 if ny == 70 else 2) and xs == (0, CG - 1, CG, nx - 1) and (nx - 1, 1) in [g for v in p['visits'] for g in v]
    for rot in range(4):
        planted = tuple((x, C.PLANT[(i + rot) % 4]) for i, x in enumerate(xs))
        c = C.build(ny, nx, 'f64' if rot % 2 == 0 else 'f32', rot < 2, True, 'plane', 'plane', seed=700 + rot, planted=planted)
        ref = _oracle(c, 'all')
        _same(_lwa(ctx, c, 0), ref, (ny, planted))
