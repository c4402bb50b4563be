"""cpiece_records_ref (K13 restated on raw records) checked on the CPU, and the hand-built cases of test_gpu_cpiece_records.py shown
to be able to fail: against contour_pieces_ref on real records; np.interp against the separately rounded formula; every exact-sum
case against the double it names, against math.fsum and against accumulators broken on purpose; every topology against a
pointer doubling that stops two rounds early.  No GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest

import clength_ref as CR
import contour_join_ref as JR
import contour_join_periodic_ref as JP
import contour_pieces_ref as PR
import cpiece_records_ref as RR


def bits(v):
    return np.asarray(v, dtype=np.float64).view(np.int64)


def same(a, b):
    """two float64 bit for bit (the sign of a zero included)"""
    return bits(a).tolist() == bits(b).tolist()


def _noise():
    rng = np.random.default_rng(23)
    q = rng.standard_normal((37, 61))
    q[rng.random(q.shape) < 0.03] = np.nan
    lv = np.concatenate([[-9.0], np.linspace(-2.0, 2.0, 5), [np.nan]])
    return q, lv


def _records(segs):
    """per-level (e_from, e_to, pts) -> count, e_from, e_to, pts"""
    return (np.array([s[0].size for s in segs], dtype=np.uint64), np.concatenate([s[0] for s in segs]),
            np.concatenate([s[1] for s in segs]), np.concatenate([s[2] for s in segs]))


PLANES = [(latlon, periodic) for latlon in (False, True) for periodic in (False, True)]


@pytest.mark.parametrize('latlon,periodic', PLANES)
@pytest.mark.parametrize('field', ['noise', 'rows'])
def test_the_helper_agrees_with_contour_pieces_ref_on_real_records(latlon, periodic, field):
    q, lv = _noise()
    ny, nx = q.shape
    if field == 'rows':                                                      # wavy rows: on a periodic plane rings round the ring
        q = np.arange(ny, dtype=np.float64)[:, None] + 0.8 * np.sin(np.arange(nx) * (6.0 * np.pi / nx))[None, :]
        lv = np.array([3.3, 17.25, 30.5])
    y, x = CR.plane_coords(np.linspace(-60.0, 60.0, ny), np.arange(nx) * 2.5, latlon)
    period = float(x[1] - x[0]) * nx if periodic else None
    ref = PR.pieces(q, lv, y, x, latlon, period)
    cnt, ef, et, pts = _records(JP.segments(q, lv) if periodic else JR.segments(q, lv))
    got = RR.pieces(cnt, ef, et, pts, ny, nx, y, x, periodic, period or 0.0, CR.RADIUS if latlon else 0.0)
    assert len(got) == len(ref) == lv.size and sum(t.size for t, _, _ in got) > (200 if field == 'noise' else 2)
    for k, ((t, lt, at), r) in enumerate(zip(got, ref)):
        assert t.size == r.size, k
        for f in RR.INT_FIELDS + ('row_min', 'row_max'):
            assert np.array_equal(t[f], r[f]), (k, f)
        assert np.array_equal(np.isnan(t['area']), ~r['closed'])
        if latlon:
            assert (np.abs(t['length'] - r['length']) <= 1e-12 * r['length']).all(), k
            cl = r['closed']
            assert (np.abs(t['area'][cl] - r['area'][cl]) <= 1e-12 * r['area_abs'][cl]).all(), k
        else:
            assert same(t['length'], r['length']) and same(t['area'][r['closed']], r['area'][r['closed']]), k
        for p in range(t.size):                                              # the terms returned are the ones summed
            assert len(lt[p]) <= t['nseg'][p] == len(at[p])
    if field == 'rows':
        assert all((t['winding'] != 0).all() and t['closed'].all() for t, _, _ in got) == periodic


@pytest.mark.parametrize('periodic', [False, True])
def test_np_interp_is_the_separately_rounded_formula_on_these_records(periodic):
    """contour_pieces_ref takes its coordinates from np.interp, the kernel from interp_at's sub, mul, add: here they are the
    same doubles, so the field tests may ask for the Cartesian areas bit for bit"""
    q, lv = _noise()
    ny, nx = q.shape
    _, _, _, pts = _records(JP.segments(q, lv) if periodic else JR.segments(q, lv))
    for latlon in (False, True):
        y, x = CR.plane_coords(np.linspace(-60.0, 60.0, ny), np.arange(nx) * 2.5, latlon)
        xe = RR.x_nodes(x, periodic, float(x[1] - x[0]) * nx)
        for col, F in ((0, y), (2, y), (1, xe), (3, xe)):
            assert same(np.interp(pts[:, col], np.arange(F.size), F), RR.interp_nodes(pts[:, col], F)), (latlon, col)
    frac = np.array([0.0, 0.5, 1.0 / 3.0, 1.0 - 2.0 ** -53, 1.0, 1.5, 2.0])
    F = np.array([0.1, 0.7, 2.3])
    assert same(RR.interp_nodes(frac, F), np.interp(frac, np.arange(3), F))
    assert same(RR.interp_nodes([1.0 / 3.0], F), [(0.7 - 0.1) * (1.0 / 3.0) + 0.1])


def test_window_and_cut():
    x = RR.exact_plane([1.0, 0.25])
    w = RR.window(RR.EXACT_Y, x)
    assert w == dict(length_top=13, length_bottom=-147, area_top=13, area_bottom=-147)   # 1.118.. and 1.0000001: 2^1 (0.5..), + 12
    assert RR.window([0.0, 1.0], np.arange(4.0) * 0.5)['length_top'] == 13 and RR.window([0.0, 0.25], np.arange(4.0) * 0.5)['length_top'] == 12
    assert RR.window([0.0, 1.0], np.arange(4.0), True, 7.0)['area_top'] == 3 + 12          # the seam cell, 4 wide, counts
    assert RR.window([0.0, 1.0], np.arange(4.0), radius=2.0)['length_top'] == 2 + 12       # 3.2 on the sphere
    assert RR.window([0.0, 0.0], [0.0, 0.0])['length_top'] == -800
    assert RR.cut(1.5, -1) == 1.5 and RR.cut(1.75, -1) == 1.5 and RR.cut(-1.75, -1) == -1.5 and RR.cut(0.25, -1) == 0.0
    assert RR.cut(RR.ONE_UP, -52) == RR.ONE_UP and RR.cut(RR.ONE_UP, -51) == 1.0


# ------------------------------------------------------------------ accumulators, sound and broken
def running_sum(terms):
    s = 0.0
    for t in terms:
        s += float(t)
    return s


round_exact, limb_sum, DEFECTS = RR.round_exact, RR.limb_sum, RR.DEFECTS      # the limb model lives beside the cases it is run on
TOP = 13                                # the windows of every exact case (asserted below)


def orders(terms):
    t = list(terms)
    return [t, t[::-1], sorted(t, key=abs), sorted(t, key=abs, reverse=True)]


def all_cases():
    """every exact-sum case of the GPU tests: name -> terms of one piece"""
    cases = {k: v[0] for k, v in RR.exact_cases().items()}
    cases['every shift'] = RR.every_shift_terms()
    for k, t in enumerate(RR.every_shift_terms()):
        cases['shift %d alone' % k] = [t]
    cases['all ones'] = RR.all_ones_terms()
    for k, t in enumerate(RR.all_ones_terms()):
        cases['ones %d alone' % k] = [t]
    rt = RR.random_terms()
    cases['random ring'] = rt
    for p in range(7):
        cases['random piece %d' % p] = rt[p::7]
    bottom = TOP - 160
    cases['bottom of the window'], cases['whole at the bottom'] = RR.bottom_terms(bottom)
    return cases


def test_every_exact_case_names_what_fsum_returns_and_a_running_sum_does_not():
    for name, (terms, want) in RR.exact_cases().items():
        assert same(math.fsum(terms), want), name
        assert same(round_exact(sum(Fraction(t) for t in terms)), want), name
        rec = RR.exact_records([terms])
        w = RR.window(rec['ycoord'], rec['xcoord'])
        assert w['length_top'] == w['area_top'] == TOP, name
        assert all(RR.cut(t, w['area_bottom']) == t and abs(t) < 2.0 ** TOP for t in terms), name     # whole inside the window
    # some order of a running float64 sum misses the value (never with two terms: such a sum is rounded once either way)
    for name in ('absorption', 'sticky lifts the tie', 'sticky pulls the tie down', 'negative sticky', 'cancellation', 'borrow, sticky'):
        terms, want = RR.exact_cases()[name]
        assert any(not same(running_sum(o), want) for o in orders(terms)), name
    a = RR.exact_cases()['absorption'][0]
    assert running_sum(a) == 1.0 and a[0] == 1.0 and math.fsum(a) == 1.0 + 2.0 ** -48
    sh = RR.every_shift_terms()
    assert not same(running_sum(sh[::-1]), math.fsum(sh)) or not same(running_sum(sh), math.fsum(sh))
    rt = RR.random_terms()
    assert len(rt) == 3000 and not same(running_sum(rt), math.fsum(rt))
    assert max(abs(t) for t in rt) < 2.0 and min(abs(t) for t in rt) >= 2.0 ** -90


def test_the_limb_model_is_exact_and_every_defect_is_caught_and_every_case_catches_one():
    """the sound mechanism returns fsum on every case; each broken one fails some case; and every case with more than one term fails
    under some broken accumulator (the running float64 sum among them) -- so each GPU comparison can tell"""
    cases = all_cases()
    caught = {d: [] for d in DEFECTS + ('a running float64 sum',)}
    for name, terms in cases.items():
        bottom = TOP - 160
        want = math.fsum([RR.cut(t, bottom) for t in terms])
        assert same(limb_sum(terms, TOP), want), name
        assert same(limb_sum(terms[::-1], TOP), want), name
        for d in DEFECTS:
            if not same(limb_sum(terms, TOP, d), want):
                caught[d].append(name)
        if any(not same(running_sum(o), want) for o in orders(terms)):
            caught['a running float64 sum'].append(name)
    for d, names in caught.items():
        assert names, 'no case catches: ' + d
    hit = set(n for names in caught.values() for n in names)
    for name, terms in cases.items():
        # (one term alone is returned as it is; the bottom case is about the cut, shown below)
        assert name in hit or len(terms) == 1 or name == 'bottom of the window', name + ': no broken accumulator fails this case'
    # the cases written for a defect do catch it
    assert 'absorption' in caught['a running float64 sum'] and 'random ring' in caught['a running float64 sum']
    assert {'tie to even, down', 'negative tie to even'} <= set(caught['ties away from zero'])
    assert {'tie to even, up', 'borrow, tie to even'} <= set(caught['ties toward zero'])
    assert {'sticky lifts the tie', 'negative sticky'} <= set(caught['no sticky bit'])
    assert {'borrow, sticky', 'sticky pulls the tie down'} <= set(caught['a running float64 sum'])
    assert {'all limbs negative', 'negative borrow', 'negative sticky'} <= set(caught['no borrow on a negative sum'])
    assert {'absorption', 'borrow through three limbs', 'borrow, exact'} <= set(caught['a carry lost between limbs'])
    # a middle chunk misplaced at one shift: the sum of all the terms (about 2) rounds it away, and (1 + 2^-52) 2^-k has an empty
    # middle chunk; the all-ones terms alone in a piece, 94 - k bits above the window's bottom, catch it at (94 - k) mod 32 == 17
    off = set(caught['a chunk one limb off at shift 17'])
    assert {'ones 13 alone', 'ones 45 alone', 'ones 77 alone', 'random ring'} <= off
    assert not any(n.startswith('shift') or n == 'every shift' for n in off)
    # the bottom of the window: the straddling term is cut, and the cut shows in the sum
    t = cases['bottom of the window']
    assert RR.cut(t[0], TOP - 160) == math.ldexp(1.0, TOP - 160 + 20) != t[0] and RR.cut(t[1], TOP - 160) == t[1]
    assert RR.cut(cases['whole at the bottom'][0], TOP - 160) == cases['whole at the bottom'][0]
    assert not same(math.fsum(t), math.fsum([RR.cut(v, TOP - 160) for v in t]))


# ------------------------------------------------------------------ labelling: pointer doubling, sound and two rounds short
def doubling_walker(short=0):
    """RR.walk's pieces from synchronous pointer doubling, as the header of K13 describes it: label' = min over self, next and
    prev, next' = next[next], prev' = prev[prev], R = ceil(log2(n)) + 1 rounds (less `short`); pieces by the final label, open where
    the root's prev has run off the head"""
    def walker(e_from, e_to, E):
        ef, et = np.asarray(e_from, dtype=np.int64), np.asarray(e_to, dtype=np.int64)
        n = ef.size
        if n == 0:
            return []
        tab = np.full(E, -1, dtype=np.int64)
        tab[ef] = np.arange(n)
        nxt = tab[et]
        prv = np.full(n, -1, dtype=np.int64)
        prv[nxt[nxt >= 0]] = np.flatnonzero(nxt >= 0)
        lab = ef.copy()
        R = 1
        while (1 << (R - 1)) < n:
            R += 1
        pad = lambda a: np.concatenate([a, [-1]])                            # index -1 reads "none"
        for _ in range(max(R - short, 0)):
            big = np.concatenate([lab, [np.iinfo(np.int64).max]])
            lab = np.minimum(lab, np.minimum(big[nxt], big[prv]))
            nxt, prv = pad(nxt)[nxt], pad(prv)[prv]
        root = tab[lab]
        out = []
        for r in np.flatnonzero(root == np.arange(n)):
            out.append((np.flatnonzero(root == r).tolist(), bool(prv[r] >= 0)))
        return out
    return walker


def _tables(rec, walker):
    cnt, ef, et, pts = rec[:4]
    return RR.pieces(cnt, ef, et, pts, 8, 300, np.arange(8.0), np.arange(300.0), walker=walker)


def _int_fields(tabs):
    return [[tuple(int(v) for v in row) for row in zip(*(t[f] for f in RR.INT_FIELDS))] for t, _, _ in tabs]


TOPOLOGIES = {
    'ring per range': lambda: RR.one_chain_per_range(True),
    'open chain per range': lambda: RR.one_chain_per_range(False),
    'many pieces': lambda: RR.many_pieces(),
    'short ranges': lambda: RR.short_ranges([0, 1, 0, 63, 64, 65, 0, 130, 1, 0, 2, 0]),
    'a long range beside a short one': lambda: RR.short_ranges([2, 4097, 0, 2]),
}


@pytest.mark.parametrize('name', sorted(TOPOLOGIES))
def test_topologies_are_what_they_say_and_a_short_doubling_fails_them(name):
    rec = TOPOLOGIES[name]()
    want = _int_fields(_tables(rec, RR.walk))
    assert _int_fields(_tables(rec, doubling_walker(0))) == want
    short = _int_fields(_tables(rec, doubling_walker(2)))
    if name in ('ring per range', 'open chain per range', 'a long range beside a short one', 'short ranges'):
        assert short != want, 'two rounds fewer go unnoticed'
    if name.endswith('per range'):
        closed = name.startswith('ring')
        assert len(want) == len(rec[4]) == (152 if closed else 156)
        for w, (first, n) in zip(want, rec[4]):
            assert w == [(first, n, closed, 0)]
        # which chains two rounds fewer break.  Open: every length from 3 on, by the label when the smallest id sits at one end
        # and by the open flag (2^(R-2) links back do not fall off the head).  Rings: R has a round to spare for the open flag, a
        # ring's farthest member is n / 2 links away: only the powers of two are short of reach
        broken = set(n for w, s, (_, n) in zip(want, short, rec[4]) if w != s)
        assert broken >= ({64, 256, 4096} if closed else set(RR.CHAIN_LENGTHS) - {1, 2}), broken
    if name == 'many pieces':
        assert len(want[0]) == rec[4] == 450 and len(set(w[0] for w in want[0])) == 450
