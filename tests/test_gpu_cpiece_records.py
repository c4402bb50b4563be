"""xc_contour_pieces_dev (K13) on records the TEST built, against cpiece_records_ref: the labelling and the slots on hand-built
topologies (integers, equal), the two fixed-point sums on terms of the test's choosing (float64, equal BIT FOR BIT to math.fsum and to
the double each case names), the error return.  test_cpiece_records_host.py shows on the CPU that every case here can fail.
Nothing is compared to a tolerance but the lengths of oblique segments (the device hypot): 1e-12 of the length, K10's own bar."""
import functools
import math

import numpy as np
import pytest

import clength_ref as CR
import cpiece_records_ref as RR
from xcontour_amd import _native as nat

pytestmark = pytest.mark.gpu

NY, NX = 8, 300                         # the plane of the topology cases: E = 4800 edge ids, coordinates = indices
DEFAULT_CAP = 1 << 30


def call_records(ctx, count, e_from, e_to, pts, ny, nx, ycoord, xcoord, periodic=0, period=0.0, radius=0.0):
    """one xc_contour_pieces_dev call on host records with capacity = the number of segments -> (rc, piece_count, the eight record
    arrays as the entry wrote them, unsorted)"""
    count = np.ascontiguousarray(count, dtype=np.uint64).ravel()
    total, nr = int(count.sum()), count.size
    ins = [count, np.ascontiguousarray(e_from, dtype=np.int64), np.ascontiguousarray(e_to, dtype=np.int64),
           np.ascontiguousarray(pts, dtype=np.float64), np.ascontiguousarray(ycoord, dtype=np.float64),
           np.ascontiguousarray(xcoord, dtype=np.float64)]
    assert total > 0 and ins[1].size == ins[2].size == total and ins[3].size == 4 * total and ins[4].size == ny and ins[5].size == nx
    with ctx._temporaries(ins, [nr * 8] + [total * 8] * 8) as (dn, df, dt, dp, dy, dx, dpc, *rec):
        rc = ctx.lib.xc_contour_pieces_dev(ctx.handle, nr, dn.ptr, df.ptr, dt.ptr, dp.ptr, ny, nx, int(periodic), dy.ptr, dx.ptr,
                                           float(period), float(radius), total, dpc.ptr, *[b.ptr for b in rec])
        pc = dpc.download((nr,), np.uint64).astype(np.int64)
        if rc != 0:
            return rc, pc, None
        npiece = int(pc.sum())
        types = (np.int64, np.int64, np.int32, np.int32, np.float64, np.float64, np.float64, np.float64)
        return rc, pc, [b.download((npiece,), t) for b, t in zip(rec, types)]


def run_records(ctx, count, e_from, e_to, pts, ny, nx, ycoord, xcoord, periodic=0, period=0.0, radius=0.0, cap=None):
    """-> per range the records (RR.DTYPE) sorted by first_edge; cap: the workspace cap of this call (restored afterwards)"""
    try:
        if cap is not None:
            ctx.set_cpiece_workspace(cap)
        rc, pc, cols = call_records(ctx, count, e_from, e_to, pts, ny, nx, ycoord, xcoord, periodic, period, radius)
    finally:
        if cap is not None:
            ctx.set_cpiece_workspace(DEFAULT_CAP)
    assert rc == 0, 'xc_contour_pieces_dev returned %d' % rc
    out, p0 = [], 0
    for n in pc:
        t = np.empty(int(n), dtype=RR.DTYPE)
        for name, col in zip(RR.DTYPE.names, cols):
            t[name] = col[p0:p0 + int(n)]
        out.append(t[np.argsort(t['first_edge'], kind='stable')])
        p0 += int(n)
    return out


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


def check_tables(got, ref, what='', oblique=False):
    """the entry's tables against the helper's: every field equal, the floats bit for bit (oblique: `length` to 1e-12)"""
    assert len(got) == len(ref), what
    for r, (g, t) in enumerate(zip(got, ref)):
        t = t[0] if isinstance(t, tuple) else t
        assert g.size == t.size, '%s range %d: %d pieces, expected %d' % (what, r, g.size, t.size)
        for f in RR.INT_FIELDS:
            assert np.array_equal(g[f], t[f]), '%s range %d: %s' % (what, r, f)
        for f in ('row_min', 'row_max', 'area') + (() if oblique else ('length',)):
            assert same_bits(g[f], t[f]), '%s range %d: %s %r != %r' % (what, r, f, g[f].tolist()[:8], t[f].tolist()[:8])
        if oblique:
            assert (np.abs(g['length'] - t['length']) <= 1e-12 * t['length']).all(), '%s range %d: length' % (what, r)


def same_tables(a, b, what=''):
    assert len(a) == len(b), what
    for r, (u, v) in enumerate(zip(a, b)):
        assert u.size == v.size, (what, r)
        for f in RR.DTYPE.names:
            assert same_bits(u[f], v[f]) if u[f].dtype.kind == 'f' else np.array_equal(u[f], v[f]), '%s range %d: %s' % (what, r, f)


def index_plane():
    return dict(ny=NY, nx=NX, ycoord=np.arange(NY, dtype=np.float64), xcoord=np.arange(NX, dtype=np.float64))


# ------------------------------------------------------------------ 3a. labelling and slots
@functools.lru_cache(maxsize=None)
def chains(closed):
    rec = RR.one_chain_per_range(closed, NY, NX)
    return rec, RR.pieces(*rec[:4], **index_plane())


@pytest.mark.parametrize('cap', [None, 1], ids=['default cap', 'one range per group'])
@pytest.mark.parametrize('closed', [True, False], ids=['rings', 'open chains'])
def test_one_chain_per_range_every_length_order_and_place_of_the_smallest_id(ctx, closed, cap):
    """Chains of 1 .. 4097 segments (a ring from 2), each stored in walk order, reversed, shuffled and in stride order, with the
    smallest id at the head, the middle and the tail: one piece of n segments whose first_edge is that id.  Under the default cap
    all ranges share a group and R comes from the longest; one range per group gives every length the R of its own count."""
    (cnt, ef, et, pts, expect), ref = chains(closed)
    got = run_records(ctx, cnt, ef, et, pts, cap=cap, **index_plane())
    for r, (g, (first, n)) in enumerate(zip(got, expect)):
        assert g.size == 1 and (int(g['first_edge'][0]), int(g['nseg'][0]), bool(g['closed'][0])) == (first, n, closed), \
            'range %d: a chain of %d segments from id %d gave %r' % (r, n, first, g[list(RR.INT_FIELDS)].tolist())
    check_tables(got, ref, 'chains')
    assert all(float(g['length'][0]) == n for g, (_, n) in zip(got, expect))  # unit segments


def test_many_pieces_in_one_range_get_one_slot_each(ctx):
    cnt, ef, et, pts, npiece = RR.many_pieces(NY, NX)
    ref = RR.pieces(cnt, ef, et, pts, **index_plane())
    (got,) = run_records(ctx, cnt, ef, et, pts, **index_plane())
    assert got.size == npiece == 450
    key = lambda t: sorted(zip(t['first_edge'].tolist(), t['nseg'].tolist(), t['closed'].tolist()))
    assert key(got) == key(ref[0][0]) and len(set(got['first_edge'].tolist())) == 450
    assert sorted(got['nseg'][got['closed']].tolist()) == [2] * 300 and (got['nseg'][~got['closed']] == 1).sum() == 100
    check_tables([got], ref, 'many pieces')


SHORT = [0, 1, 0, 63, 64, 65, 0, 130, 1, 0, 2, 0]


@pytest.mark.parametrize('counts', [SHORT, [2, 4097, 0, 2]], ids=['short ranges', 'a long range beside short ones'])
def test_ranges_that_share_their_edge_ids_under_three_workspace_caps(ctx, counts):
    """every range draws the SAME edge ids, waves and blocks straddle the range boundaries, empty ranges sit in front, between and
    behind; the rounds of a group come from its largest count.  The cap moves the group boundaries and nothing else."""
    rec = RR.short_ranges(counts, NY, NX)
    ref = RR.pieces(*rec, **index_plane())
    off = np.concatenate([[0], np.cumsum(counts)])
    ids = [set(rec[1][a:b].tolist()) for a, b in zip(off[:-1], off[1:])]
    assert all(i <= max(ids, key=len) for i in ids) and sum(t.size for t, _, _ in ref) >= (60 if len(counts) > 4 else 3)   # shared ids, many pieces
    tabs = [run_records(ctx, *rec, cap=cap, **index_plane()) for cap in (None, 1, 3 * (2 * NY * NX) * 4)]
    for k, t in enumerate(tabs):
        check_tables(t, ref, 'cap %d' % k)
        same_tables(t, tabs[0], 'cap %d against the default' % k)


def test_winding_and_row_extents_on_a_periodic_plane(ctx):
    """rings that cross the seam twice forward, once each way and twice backward, an open chain that crosses it; rows 0.0,
    fractional and ny - 1"""
    nx, top = float(NX), float(NY - 1)
    fwd = lambda r: [[r, 298.5, r + 0.5, nx], [r + 0.5, 0.0, r + 0.25, 150.0]]      # ends on column nx, goes on from column 0
    back = lambda r: [[r, 149.5, r + 0.5, 0.0], [r + 0.5, nx, r + 0.25, 151.0]]     # ends on column 0, goes on from column nx
    shapes = [(fwd(0.0) + fwd(1.0), True, 2), (fwd(2.0) + back(top - 0.5), True, 0), (back(3.0) + back(4.0), True, -2),
              (fwd(5.5) + [[6.0, 10.0, 6.75, 11.0]], False, 0), (back(0.0) + [[0.5, 151.0, 0.5, 152.0]], True, -1)]
    EF, ET, PT, at = [], [], [], 0
    ids = np.random.default_rng(8).permutation(2 * NY * NX)
    for segs, closed, _ in shapes:
        ef, et = RR.chain(ids[at:at + len(segs)], closed, ids[-1 - at])
        EF.append(ef); ET.append(et); PT.append(np.array(segs)); at += len(segs)
    ef, et, pts = np.concatenate(EF), np.concatenate(ET), np.concatenate(PT)
    o = np.random.default_rng(9).permutation(ef.size)
    plane = dict(index_plane(), periodic=1, period=float(NX))
    rec = (np.array([ef.size, 0, ef.size], dtype=np.uint64), np.concatenate([ef[o], ef]), np.concatenate([et[o], et]),
           np.concatenate([pts[o], pts]))
    ref = RR.pieces(*rec, **plane)
    got = run_records(ctx, *rec, **plane)
    check_tables(got, ref, 'winding', oblique=True)
    for g in (got[0], got[2]):
        by_first = {int(f): k for k, f in enumerate(g['first_edge'])}
        at = 0
        for segs, closed, w in shapes:
            k = by_first[int(ids[at:at + len(segs)].min())]
            rows = np.array(segs)[:, [0, 2]]
            assert (bool(g['closed'][k]), int(g['winding'][k]), int(g['nseg'][k])) == (closed, w, len(segs))
            assert g['row_min'][k] == rows.min() and g['row_max'][k] == rows.max()
            at += len(segs)
        assert g['row_min'].min() == 0.0 and g['row_max'].max() == top
    # the same records on the plain plane: no winding (column nx is then past the last node and is read as the last node)
    assert all((t['winding'] == 0).all() for t in run_records(ctx, *rec, **index_plane()))


def permuted(cnt, ef, et, pts, how, rng):
    """the records of every range in another storage order"""
    idx, s0 = [], 0
    for c in np.asarray(cnt).ravel().astype(np.int64):
        loc = {'reversed': lambda: np.arange(c)[::-1], 'random': lambda: rng.permutation(c),
               'by e_to': lambda: np.argsort(et[s0:s0 + c], kind='stable')}[how]()
        idx.append(s0 + loc); s0 += int(c)
    o = np.concatenate(idx).astype(np.int64)
    return ef[o], et[o], pts[o]


@pytest.mark.parametrize('field', ['noise', 'baro'])
def test_k12_records_in_any_storage_order_give_the_same_bits(ctx, baro, field):
    """"the records do not depend on the order of the segments": K12's own records, permuted inside every range, through the C
    entry -- every field, length and area included, bit for bit that of Context.contour_pieces (K12's emission order); on the
    sphere too, where the host cannot reproduce the terms but their sum must not move"""
    if field == 'noise':
        rng = np.random.default_rng(23)
        q = rng.standard_normal((97, 301))
        q[rng.random(q.shape) < 0.03] = np.nan
        fy, fx = CR.plane_coords(np.arange(97) * 1.5 - 72.0, np.arange(301) * 1.125, False)
        lv, kw, periodic = np.concatenate([[-9.0], np.linspace(-2.0, 2.0, 8), [11.0, np.inf]]), {}, False
    else:
        q, lat, lon = baro
        q = np.asarray(q, dtype=np.float64)
        fy, fx = CR.plane_coords(lat, lon, True)
        lv, periodic = np.linspace(float(q.min()), float(q.max()), 21), True
        kw = dict(radius=CR.RADIUS, period=float(np.float64(np.deg2rad(np.float32(360.0)))))
    ny, nx = q.shape
    pc, tab = ctx.contour_pieces(q[None], lv, fy, fx, **kw)
    cnt, ef, et, pts = ctx.contour_segments(q[None], lv, periodic=periodic)
    assert tab.size > (2000 if field == 'noise' else 20) and (tab['nseg'].sum() == cnt.sum())
    rng = np.random.default_rng(4)
    for how in ('reversed', 'random', 'by e_to'):
        pf, pt, pp = permuted(cnt, ef, et, pts, how, rng)
        assert not np.array_equal(pf, ef)
        got = run_records(ctx, cnt.ravel(), pf, pt, pp, ny, nx, fy, fx, int(periodic), kw.get('period', 0.0), kw.get('radius', 0.0))
        assert np.array_equal([g.size for g in got], pc.ravel().astype(np.int64)), how
        allgot = np.concatenate(got)
        for f in RR.DTYPE.names:
            a, b = allgot[f], tab[f]
            assert same_bits(a, b) if a.dtype.kind == 'f' else np.array_equal(a, b), '%s, records %s: %s' % (field, how, f)


# ------------------------------------------------------------------ 3b. exact sums on a Cartesian plane
def run_exact(ctx, groups, order=None, cutting=False):
    """rings of the given signed terms on an exact_plane through the entry -> (table, helper's table, windows).  The helper sums
    with math.fsum (cutting: of the terms cut at the window's bottom, as the header documents)."""
    rec = RR.exact_records(groups, order=order)
    args = (rec['count'], rec['e_from'], rec['e_to'], rec['pts'], rec['ny'], rec['nx'], rec['ycoord'], rec['xcoord'])
    w = RR.window(rec['ycoord'], rec['xcoord'])
    fs = {}
    if cutting:
        assert w['length_bottom'] == w['area_bottom']
        fs = dict(fsum=lambda ts: math.fsum(RR.cut(t, w['area_bottom']) for t in ts))
    ((ref, lt, at),) = RR.pieces(*args, **fs)
    flat = [t for g in groups for t in g if t != 0.0]
    assert sorted(abs(t) for t in flat) == sorted(float(v) for ts in lt for v in ts)          # the terms are the ones asked for
    assert sorted(flat) == sorted(float(v) for ts in at for v in ts if v != 0.0)
    (got,) = run_records(ctx, *args)
    assert got.size == len(groups) and got['closed'].all()
    return got, ref, w


def check_sums(got, ref, groups, what=''):
    for p, g in enumerate(groups):
        for f in ('length', 'area'):
            assert same_bits(got[f][p], ref[f][p]), '%s piece %d: %s %r, fsum %r (%d terms)' % (what, p, f, float(got[f][p]), float(ref[f][p]), len(g))


def test_named_exact_sums(ctx):
    """absorption, ties to even either way, the sticky bit, cancellation, negative limbs, borrows, a ring that cancels to +0: the
    area is the double each case names and the length is fsum of the magnitudes, bit for bit"""
    cases = RR.exact_cases()
    groups = [c[0] for c in cases.values()]
    got, ref, w = run_exact(ctx, groups)
    assert w['length_top'] == w['area_top'] == 13
    for p, (name, (terms, want)) in enumerate(cases.items()):
        assert all(abs(t) < 2.0 ** 13 and RR.cut(t, w['area_bottom']) == t for t in terms), name    # whole inside both windows
        assert same_bits(ref['area'][p], want) and same_bits(got['area'][p], want), \
            '%s: area %r (%s), expected %r' % (name, float(got['area'][p]), float(got['area'][p]).hex(), want)
        assert same_bits(got['length'][p], math.fsum(abs(t) for t in terms)), '%s: length %r' % (name, float(got['length'][p]))
    check_sums(got, ref, groups, 'named')
    assert math.copysign(1.0, got['area'][list(cases).index('cancels to +0')]) == 1.0


def test_every_shift_and_every_limb(ctx):
    """(1 + 2^-52) 2^-k, k = 0..95, and (1 - 2^-53) 2^-k, k = 0..94 (no empty chunk): all in one piece, and one piece per term
    -- a one-term sum returns the term itself"""
    sh, ones = RR.every_shift_terms(), RR.all_ones_terms()
    groups = [sh, ones] + [[t, 0.0] for t in sh] + [[-t, 0.0] for t in ones]
    got, ref, w = run_exact(ctx, groups)
    assert w['area_bottom'] == -147 and RR.cut(sh[-1], -147) == sh[-1] and RR.cut(ones[-1], -147) == ones[-1]
    check_sums(got, ref, groups, 'shifts')
    for p, g in enumerate(groups[2:], 2):
        assert got['area'][p] == g[0] and got['length'][p] == abs(g[0]) and got['nseg'][p] == 2, (p, g[0].hex())


def test_the_bottom_of_the_window(ctx):
    """a term whose last bit is the window's last survives whole; a 53-bit term that straddles the bottom is cut there: the sum is
    fsum of the cut terms.  (One cell of width 1 fixes both windows: top 13, bottom -147.)"""
    straddling, whole = RR.bottom_terms(-147)
    groups = [straddling, whole + [0.0], [-v for v in straddling], [1.0, 0.0]]
    got, ref, w = run_exact(ctx, groups, cutting=True)
    assert w['length_bottom'] == w['area_bottom'] == -147
    check_sums(got, ref, groups, 'bottom')
    assert got['area'][1] == whole[0] == got['length'][1]
    cut_sum = math.ldexp(1.0, -127) + math.ldexp(1.0, -147)
    assert got['area'][0] == cut_sum == got['length'][0] == -got['area'][2] and cut_sum != math.fsum(straddling)


def test_a_term_above_the_window_makes_its_piece_nan_and_no_other(ctx):
    """16400 unit cells, ycoord (1, 0.5): both windows end at 2^13.  A segment over 4096 cells (2^12) is summed exactly; one over
    8192 (2^13 itself) or 16384 cells is not: NaN for that sum of that piece.  Along row 1 the area term of 8192 cells is 4096:
    inside, while the length is not."""
    nx = 16400
    x = np.arange(nx, dtype=np.float64)
    w = RR.window(RR.EXACT_Y, x)
    assert w['length_top'] == w['area_top'] == 13
    span = lambda n, row=0.0: [row, float(n), row, 0.0]                        # length n, area term +n y[row]
    unit = [0.0, 7.0, 0.0, 6.0]
    shapes = [([span(4096), unit], 4097.0, 4097.0), ([span(16384), unit], math.nan, math.nan), ([span(8192), unit], math.nan, math.nan),
              ([span(8192, 1.0), unit], math.nan, 4097.0), ([unit, unit, unit], 3.0, 3.0), ([span(4096, 1.0), span(4095)], 8191.0, 6143.0)]
    EF, ET, PT, at = [], [], [], 0
    for segs, _, _ in shapes:
        ef, et = RR.chain(np.arange(at, at + len(segs)) * 3 + 1, True)
        EF.append(ef); ET.append(et); PT.append(np.array(segs)); at += len(segs)
    args = (np.array([at], dtype=np.uint64), np.concatenate(EF), np.concatenate(ET), np.concatenate(PT), 2, nx, RR.EXACT_Y, x)
    ((ref, lt, art),) = RR.pieces(*args)
    (got,) = run_records(ctx, *args)
    assert got.size == len(shapes)
    for p, (segs, length, area) in enumerate(shapes):
        over_l, over_a = bool((np.abs(lt[p]) >= 2.0 ** 13).any()), bool((np.abs(art[p]) >= 2.0 ** 13).any())
        assert over_l == math.isnan(length) and over_a == math.isnan(area), p
        assert same_bits(got['length'][p], length) and same_bits(got['area'][p], area), \
            'piece %d: length %r area %r, expected %r %r' % (p, float(got['length'][p]), float(got['area'][p]), length, area)
        if not over_l:
            assert same_bits(ref['length'][p], length)
        if not over_a:
            assert same_bits(ref['area'][p], area)


def test_random_terms_in_one_ring_in_seven_pieces_and_permuted(ctx):
    rt = RR.random_terms()
    rng = np.random.default_rng(10)
    for what, groups in (('one ring', [rt]), ('seven pieces', [rt[p::7] for p in range(7)])):
        got, ref, _ = run_exact(ctx, groups)
        check_sums(got, ref, groups, what)
        again, _, _ = run_exact(ctx, groups, order=rng.permutation(len(rt)))
        same_tables([again], [got], what + ', permuted')


@pytest.mark.parametrize('periodic', [0, 1])
def test_coordinate_interpolation_is_rounded_operation_by_operation(ctx, periodic):
    """end points at 0.5, 1/3, 1 - 2^-53 and on nodes, on a non-uniform plane; on a periodic plane segments on the seam cell, whose
    far column nx lies at xcoord[0] + period.  The area of every ring bit for bit; the length bit for bit where every segment is
    axis-aligned (hypot(d, 0) = |d|), else to 1e-12."""
    y, x, period = np.array([0.1, 0.7, 2.3]), np.array([0.3, 1.0, 2.5, 3.25, 5.0]), 6.7
    third, last = 1.0 / 3.0, 1.0 - 2.0 ** -53
    aligned = [[0.5, 0.5, 0.5, 1.0 + third], [third, 2.0 + last, third, 0.25], [1.0 + last, 3.0, 1.0 + third, 3.0], [2.0, third, 2.0, 3.5],
               [last, 2.5, last, 2.5]]
    oblique = [[0.5, 0.5, 1.0 + third, 2.0 + last], [1.0 + third, 2.0 + last, 2.0, 4.0], [2.0, 4.0, last, third], [third, last, 0.5, 0.5]]
    pieces = [(aligned, True), (oblique, False)]
    if periodic:
        pieces += [([[0.5, 4.0, 0.5, 5.0], [0.5, 0.0, 0.5, third], [third, 4.5, third, 4.0 + third], [1.5, 5.0, 1.5, 4.0 + last]], True),
                   ([[0.0, 4.5, 1.0 + third, 5.0], [1.0 + third, 0.0, 2.0, 4.0 + third], [2.0, 4.0 + last, 0.5, 4.0]], False)]
    EF, ET, PT, at = [], [], [], 0
    for segs, _ in pieces:
        ef, et = RR.chain(np.arange(at, at + len(segs)), True)
        EF.append(ef); ET.append(et); PT.append(np.array(segs)); at += len(segs)
    args = (np.array([at], dtype=np.uint64), np.concatenate(EF), np.concatenate(ET), np.concatenate(PT), 3, 5, y, x, periodic, period)
    ((ref, lt, art),) = RR.pieces(*args)
    (got,) = run_records(ctx, *args)
    assert got.size == len(pieces)
    for p, (segs, exact) in enumerate(pieces):
        assert same_bits(got['area'][p], ref['area'][p]), 'piece %d: area %r, fsum %r' % (p, float(got['area'][p]), float(ref['area'][p]))
        if exact:
            assert same_bits(got['length'][p], ref['length'][p]), 'piece %d: length %r, fsum %r' % (p, float(got['length'][p]), float(ref['length'][p]))
        else:
            assert abs(got['length'][p] - ref['length'][p]) <= 1e-12 * ref['length'][p], p
    # one value by hand: the seam cell runs from x[4] = 5.0 to x[0] + period = 7.0
    if periodic:
        assert float(RR.interp_nodes([4.5], RR.x_nodes(x, True, period))[0]) == (7.0 - 5.0) * 0.5 + 5.0 == 6.0


# ------------------------------------------------------------------ 3c. the error return
@pytest.mark.parametrize('which,value', [('e_from', 2 * NY * NX), ('e_to', -1)])
def test_an_edge_id_out_of_range_is_refused_and_the_next_call_is_right(ctx, which, value):
    cnt, ef, et, pts, npiece = RR.many_pieces(NY, NX)
    ref = RR.pieces(cnt, ef, et, pts, **index_plane())
    bad_f, bad_t = ef.copy(), et.copy()
    (bad_f if which == 'e_from' else bad_t)[517] = value
    rc, pc, cols = call_records(ctx, cnt, bad_f, bad_t, pts, **index_plane())
    assert rc == nat.XC_EBADARG and cols is None and pc.shape == (1,)         # piece_count was written and can be read
    check_tables(run_records(ctx, cnt, ef, et, pts, **index_plane()), ref, 'the call after the refused one')
