"""xc_contour_overturning_dev (K16) on records the TEST built, against coverturn_ref: every output equal -- the integers, the rows
bit for bit, NaN in the same places.  test_coverturn_host.py shows on the CPU that the restatement can tell a wrong rule.  Every
call hands the entry output arrays filled with a pattern and followed by guard elements: on XC_OK every element is written and
every guard intact, on a refusal before the first launch nothing is touched."""
import functools

import numpy as np
import pytest

import coverturn_ref as OR
import cpiece_records_ref as RR
from xcontour_amd import _native as nat

pytestmark = pytest.mark.gpu

NY = 8
DEFAULT_CAP = 1 << 30
GUARD = 16                                  # elements behind every output
TYPES = (np.int32, np.float64, np.float64, np.int32, np.int64, np.int64, np.int32)
PATTERN = {np.int32: 0x5a5a5a5a, np.int64: 0x5a5a5a5a5a5a5a5a, np.float64: -1.2345e300}


def call_records(ctx, count, e_from, e_to, pts, ny, nx, periodic, select):
    """one xc_contour_overturning_dev call on host records -> (rc, the seven outputs as OR.FIELDS names them, untouched: every
    output still holds the pattern it was given); the guards are checked here"""
    count = np.ascontiguousarray(count, dtype=np.uint64).ravel()
    total, nr = int(count.sum()), count.size
    ins = [count, np.ascontiguousarray(e_from, dtype=np.int64), np.ascontiguousarray(e_to, dtype=np.int64),
           np.ascontiguousarray(pts, dtype=np.float64)]
    assert ins[1].size == ins[2].size == total and ins[3].size == 4 * total
    sizes = [nr * nx] * 3 + [nr] * 4
    outs = [np.full(n + GUARD, PATTERN[t], dtype=t) for n, t in zip(sizes, TYPES)]
    with ctx._temporaries(ins + outs, []) as (dn, df, dt, dp, *dout):
        rc = ctx.lib.xc_contour_overturning_dev(ctx.handle, nr, dn.ptr, df.ptr, dt.ptr, dp.ptr, ny, nx, int(periodic), int(select),
                                                *[b.ptr for b in dout])
        back = [b.download((n + GUARD,), t) for b, n, t in zip(dout, sizes, TYPES)]
    for name, b, n, t in zip(OR.FIELDS, back, sizes, TYPES):
        assert (b[n:].view(np.int64 if t == np.float64 else t) == np.full(GUARD, PATTERN[t], dtype=t).view(np.int64 if t == np.float64 else t)).all(), \
            'the guard behind %s was written' % name
    untouched = all((b[:n].view(np.uint8) == np.full(n, PATTERN[t], dtype=t).view(np.uint8)).all() for b, n, t in zip(back, sizes, TYPES))
    res = {name: b[:n].reshape((nr, nx) if k < 3 else (nr,)) for k, (name, b, n) in enumerate(zip(OR.FIELDS, back, sizes))}
    return rc, res, untouched


def run_records(ctx, rec, nx, periodic, select, cap=None):
    try:
        if cap is not None:
            ctx.set_cpiece_workspace(cap)
        rc, res, _ = call_records(ctx, *rec[:4], NY, nx, periodic, select)
    finally:
        if cap is not None:
            ctx.set_cpiece_workspace(DEFAULT_CAP)
    assert rc == 0, 'xc_contour_overturning_dev returned %d' % rc
    return res


def check(got, rec, nx, periodic, select, what=''):
    ref = OR.overturning(*rec[:4], NY, nx, periodic, select)
    assert OR.differences(got, ref) == [], '%s (periodic %d, select %d): %r differ' % (what, periodic, select, OR.differences(got, ref))
    return ref


def every_select(ctx, rec, nx, what='', cap=None):
    """the records on the plain plane ('all') and on the ring (all three selects), each against the restatement"""
    out = {}
    for periodic, select in ((0, 0), (1, 0), (1, 1), (1, 2)):
        got = run_records(ctx, rec, nx, periodic, select, cap=cap)
        out[periodic, select] = (got, check(got, rec, nx, periodic, select, what))
    return out


def seam_pts(n, nx, rng, seam=0.2):
    """n end-point records with rows on eighths in [0, NY - 1] and columns on quarters in [0, nx), a share of the start and of the end
    columns ON the seam cell's right edge (column nx): the winding of a ring is whatever the seam count says"""
    pts = np.stack([rng.integers(0, 8 * (NY - 1) + 1, n) / 8.0, rng.integers(0, 4 * nx, n) / 4.0,
                    rng.integers(0, 8 * (NY - 1) + 1, n) / 8.0, rng.integers(0, 4 * nx, n) / 4.0], axis=1)
    pts[rng.random(n) < seam, 1] = float(nx)
    pts[rng.random(n) < seam, 3] = float(nx)
    return pts


def ring_pts(n, nx, rng, w):
    """the same, with exactly |w| seam columns, on the end points (w > 0) or on the start points: a ring of winding w"""
    pts = seam_pts(n, nx, rng, seam=0.0)
    pts[rng.choice(n, abs(w), replace=False), 3 if w > 0 else 1] = float(nx)
    return pts


# ------------------------------------------------------------------ chains and rings of every length and order
LENGTHS = (1, 2, 63, 64, 65, 4097)
WINDINGS = (-2, -1, 0, 1, 2)


@functools.lru_cache(maxsize=None)
def chains(closed, nx=300):
    """one chain per range: every length in the four storage orders; a ring's winding runs through -2 .. +2 (as far as its length allows)"""
    rng = np.random.default_rng(31)
    E = 2 * NY * nx
    cnt, EF, ET, PT, wind = [], [], [], [], []
    for n in LENGTHS:
        for name, order in RR.storage_orders(n, rng).items():
            ids = rng.permutation(E)[:n + 1]
            ef, et = RR.chain(ids[:n], closed, int(ids[n]))
            w = int(np.clip(WINDINGS[len(cnt) % 5], -n, n))
            pts = ring_pts(n, nx, rng, w)
            cnt.append(n); EF.append(ef[order]); ET.append(et[order]); PT.append(pts[order]); wind.append(w)
    return np.array(cnt, dtype=np.uint64), np.concatenate(EF), np.concatenate(ET), np.concatenate(PT), wind


@pytest.mark.parametrize('cap', [None, 1], ids=['default cap', 'one range per group'])
@pytest.mark.parametrize('closed', [True, False], ids=['rings', 'open chains'])
def test_one_chain_per_range_every_length_order_and_winding(ctx, closed, cap):
    rec = chains(closed)
    res = every_select(ctx, rec, 300, 'chains', cap=cap)
    cnt, wind = rec[0].astype(np.int64), np.array(rec[4])
    got, ref = res[1, 2]
    if closed:
        assert set(wind.tolist()) == set(WINDINGS)
        assert np.array_equal(got['main_winding'], wind) and np.array_equal(got['main_nseg'], np.where(wind != 0, cnt, 0))
        assert np.array_equal(got['nsel'], (wind != 0).astype(np.int32))
        assert np.array_equal(res[1, 0][0]['ncross'].sum(axis=1), [int((rec[1][a:b] & 1).sum()) for a, b in zip(np.cumsum(cnt) - cnt, np.cumsum(cnt))])
    else:
        assert not got['nsel'].any() and not got['ncross'].any() and np.isnan(got['row_lo']).all() and (got['main_first_edge'] == -1).all()
        assert (res[0, 0][0]['nsel'] == 1).all()


# ------------------------------------------------------------------ many pieces, shared ids, caps
def with_seam_pts(rec, nx, seed):
    return rec[:3] + (seam_pts(rec[1].size, nx, np.random.default_rng(seed)),)


def test_450_pieces_in_one_range(ctx):
    cnt, ef, et, _, npiece = RR.many_pieces(NY, 300)
    rec = with_seam_pts((cnt, ef, et), 300, 32)
    res = every_select(ctx, rec, 300, 'many pieces')
    assert npiece == 450 and res[0, 0][0]['nsel'].tolist() == [450] == res[1, 0][0]['nsel'].tolist()
    assert 50 < res[1, 1][0]['nsel'][0] < 300 and res[1, 2][0]['nsel'].tolist() == [1]      # the two-segment rings with a seam count != 0


SHORT = [0, 1, 0, 63, 64, 65, 0, 130, 1, 0, 2, 0]


@pytest.mark.parametrize('counts,nx', [(SHORT, 63), (SHORT, 64), (SHORT, 65), ([2, 4097, 0, 2], 300)],
                         ids=['short ranges, nx 63', 'nx 64', 'nx 65', 'a long range beside short ones'])
def test_ranges_that_share_their_edge_ids_under_three_workspace_caps(ctx, counts, nx):
    """every range draws the SAME edge ids; waves and blocks straddle the range boundaries (ranges of 1 and 63 segments share one
    wave); empty ranges sit in front, between and behind; a range's row of ncross ends inside, on and past a wave of the init and
    finish passes.  The cap moves the group boundaries and nothing else."""
    rec = with_seam_pts(RR.short_ranges(counts, NY, nx), nx, 33)
    runs = [every_select(ctx, rec, nx, 'cap %r' % cap, cap=cap) for cap in (None, 1, 3 * (2 * NY * nx) * 4)]
    for k, res in enumerate(runs[1:], 1):
        for key, (got, _) in res.items():
            assert OR.differences(got, runs[0][key][0]) == [], 'cap %d against the default, %r' % (k, key)
    got = runs[0][1, 0][0]
    empty = np.array(counts) == 0
    assert (got['ncross'][empty] == 0).all() and np.isnan(got['row_lo'][empty]).all() and (got['main_first_edge'][empty] == -1).all()
    assert got['ncross'][~empty].sum() > 0


# ------------------------------------------------------------------ ties, column 0
def test_an_exact_tie_of_nseg_and_crossings_on_column_0(ctx):
    """two rings of three segments, winding +1 and -1, and a longer ring of winding 0: 'main' takes the ring whose first_edge is the
    smaller, wherever it is stored.  Both rings start segments on V(r, 0) -- id 2 r nx + 1, cell 0's left edge and the seam cell's
    right edge -- which is column 0, counted once per vertex."""
    nx = 64
    V = lambda r, c: 2 * (r * nx + c) + 1
    H = lambda r, c: 2 * (r * nx + c)
    a_ids, b_ids, z_ids = [V(3, 0), H(3, 5), V(2, 63)], [V(1, 0), V(5, 0), H(6, 1)], [V(0, 0), V(0, 7), H(1, 7), V(1, 9)]
    a_pts = [[3.5, 0.0, 3.0, 5.5], [3.0, 5.5, 2.25, 63.0], [2.25, 63.0, 3.5, 64.0]]           # ends on column nx: +1
    b_pts = [[1.5, 64.0, 5.125, 0.0], [5.125, 0.0, 6.0, 1.5], [6.0, 1.5, 1.5, 0.0]]           # starts on column nx: -1
    z_pts = [[0.5, 0.0, 0.25, 7.0], [0.25, 7.0, 1.0, 7.5], [1.0, 7.5, 1.75, 9.0], [1.75, 9.0, 0.5, 0.0]]
    for first, second in ((0, 1), (1, 0)):
        rings = [(a_ids, a_pts), (b_ids, b_pts)]
        rings = [rings[first], rings[second], (z_ids, z_pts)]
        ef = np.concatenate([RR.chain(i, True)[0] for i, _ in rings])
        et = np.concatenate([RR.chain(i, True)[1] for i, _ in rings])
        rec = (np.array([10], dtype=np.uint64), ef, et, np.array(sum((p for _, p in rings), [])))
        res = every_select(ctx, rec, nx, 'tie')
        main = res[1, 2][0]
        assert (main['main_first_edge'].tolist(), main['main_nseg'].tolist(), main['main_winding'].tolist()) == ([V(1, 0)], [3], [-1])
        assert main['ncross'][0, 0] == 2 and main['ncross'].sum() == 2 and (main['row_lo'][0, 0], main['row_hi'][0, 0]) == (1.5, 5.125)
        circ = res[1, 1][0]
        assert circ['nsel'].tolist() == [2] and circ['ncross'][0, 0] == 3 and circ['ncross'][0, 63] == 1 and circ['row_lo'][0, 63] == 2.25
        every = res[1, 0][0]
        assert every['nsel'].tolist() == [3] and every['ncross'][0, 0] == 4 and every['row_lo'][0, 0] == 0.5 and every['ncross'][0, 9] == 1


# ------------------------------------------------------------------ refusals
def test_a_selection_on_a_plain_plane_is_refused_and_nothing_is_written(ctx):
    rec = chains(True)
    for select in (1, 2, 3, -1):
        rc, _, untouched = call_records(ctx, *rec[:4], NY, 300, 0, select)
        assert rc == nat.XC_EBADARG and untouched, select
    rc, _, untouched = call_records(ctx, *rec[:4], NY, 300, 1, 3)
    assert rc == nat.XC_EBADARG and untouched


def pieces_call(ctx, cnt, ef, et, pts, nx):
    """xc_contour_pieces_dev on the index plane -> the (first_edge, nseg, closed) of every piece, sorted"""
    total = int(cnt.sum())
    ins = [np.ascontiguousarray(cnt, dtype=np.uint64), ef, et, np.ascontiguousarray(pts), np.arange(NY, dtype=np.float64), np.arange(nx, dtype=np.float64)]
    with ctx._temporaries(ins, [8] + [total * 8] * 8) as (dn, df, dt, dp, dy, dx, dpc, *rec):
        rc = ctx.lib.xc_contour_pieces_dev(ctx.handle, 1, dn.ptr, df.ptr, dt.ptr, dp.ptr, NY, nx, 0, dy.ptr, dx.ptr, 0.0, 0.0, total, dpc.ptr,
                                           *[b.ptr for b in rec])
        assert rc == 0
        n = int(dpc.download((1,), np.uint64)[0])
        cols = [b.download((n,), t) for b, t in zip(rec[:3], (np.int64, np.int64, np.int32))]
    return sorted(zip(*[c.tolist() for c in cols]))


@pytest.mark.parametrize('which,value', [('e_from', 2 * NY * 300), ('e_to', -1)])
def test_an_edge_id_out_of_range_is_refused_and_the_table_is_handed_on_clean(ctx, which, value):
    cnt, ef, et, pts, npiece = RR.many_pieces(NY, 300)
    bad_f, bad_t = ef.copy(), et.copy()
    (bad_f if which == 'e_from' else bad_t)[517] = value
    rc, _, _ = call_records(ctx, cnt, bad_f, bad_t, pts, NY, 300, 1, 2)
    assert rc == nat.XC_EBADARG
    (tab, _, _), = RR.pieces(cnt, ef, et, pts, NY, 300, np.arange(NY), np.arange(300))
    assert pieces_call(ctx, cnt, ef, et, pts, 300) == sorted(zip(tab['first_edge'].tolist(), tab['nseg'].tolist(), tab['closed'].astype(int).tolist()))
    got = run_records(ctx, (cnt, ef, et, pts), 300, 1, 0)                     # and K16 itself is right after the refused call
    check(got, (cnt, ef, et, pts), 300, 1, 0, 'the call after the refused one')
