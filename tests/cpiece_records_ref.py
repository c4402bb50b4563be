"""K13 (xc_contour_pieces_dev) restated on RAW RECORDS, from the header's definition (include/xcontour_hip.h, K13 section) -- a helper
for the tests, no tests here.  Where contour_pieces_ref starts from a field and marching squares, this starts from the records
themselves -- count[nrange], e_from, e_to, pts[total, 4] -- so a test can hand the C entry records it built and know every term.

Pieces, per range: next(i) is the segment of the range whose e_from == e_to[i] (one dict per range).  A segment whose e_from is no
segment's e_to heads an open piece; what is left after the open pieces is rings.
Fields: first_edge (the smallest e_from), nseg, closed, winding (#(c2 == nx) - #(c1 == nx) over a ring's segments on a periodic
plane, else 0), row_min / row_max over both end points of every segment.
Coordinates (interp_nodes): F[j] when the index is on node j, the last node included; else (F[j+1] - F[j]) * (x - j) + F[j] with
j = floor(x), every operation a numpy call of its own and so rounded on its own: no fused multiply-add can enter, which np.interp
does not promise.  Column nx of a periodic plane is xcoord[0] + period.
Terms: length np.hypot(x1 - x2, y1 - y2), nothing for a segment whose end points coincide in index space; area
0.5 * ((ya + yb) * (x1 - x2)), NaN for an open piece.  radius > 0: clength_ref.haversine and Y' = sin(Y), the sums times radius and
radius^2 (as contour_pieces_ref).  Sums: math.fsum, or the `fsum` handed in (the host tests hand in broken ones to show that the
cases can tell).  The terms of every piece are returned beside the table.

window(): the fixed-point windows of the two sums as the header and xc_binning.h state them.  cut(): a term cut at a window's bottom.
limb_sum(): the mechanism the header names in Python integers, with DEFECTS that each break one step of it -- the host tests of K13, K17
and K18 run it on their windows to show that the reference is that mechanism and that their term lists can tell a broken one.
The builders at the end make the records of the hand-built cases; the host tests and the GPU tests share them.
"""
import math
from fractions import Fraction

import numpy as np

import clength_ref as CR

DTYPE = np.dtype([('first_edge', np.int64), ('nseg', np.int64), ('closed', np.bool_), ('winding', np.int32),
                  ('length', np.float64), ('area', np.float64), ('row_min', np.float64), ('row_max', np.float64)])
INT_FIELDS = ('first_edge', 'nseg', 'closed', 'winding')


def interp_nodes(idx, F):
    """F at the index-space positions idx: the node value on a node, else the slope formula on the node floor(idx), each operation
    rounded separately"""
    idx = np.asarray(idx, dtype=np.float64)
    F = np.asarray(F, dtype=np.float64)
    j0 = np.clip(np.floor(idx).astype(np.int64), 0, F.size - 1)
    j1 = np.minimum(j0 + 1, F.size - 1)
    j0f = j0.astype(np.float64)
    F0, F1 = F[j0], F[j1]
    d = F1 - F0
    t = idx - j0f
    p = d * t
    v = p + F0
    return np.where(idx == j0f, F0, np.where(idx == j0f + 1.0, F1, v))


def x_nodes(xcoord, periodic=False, period=0.0):
    """the node columns' coordinates: on a periodic plane column nx, at xcoord[0] + period, is one of them"""
    x = np.asarray(xcoord, dtype=np.float64)
    return np.concatenate([x, [x[0] + np.float64(period)]]) if periodic else x


def walk(e_from, e_to, E=None):
    """one range -> [(segment indices in walk order, closed), ...]: the open pieces from their heads, then the rings.  Records
    outside the contract (a repeated e_from or e_to, an id outside [0, E)) raise ValueError."""
    ef, et = [int(v) for v in e_from], [int(v) for v in e_to]
    n = len(ef)
    by_from = {e: i for i, e in enumerate(ef)}
    targets = set(et)
    if len(by_from) != n or len(targets) != n:
        raise ValueError('a repeated edge id')
    if E is not None and n and not (0 <= min(ef + et) and max(ef + et) < E):
        raise ValueError('an edge id outside [0, E)')
    seen = [False] * n
    out = []

    def follow(i):
        segs = []
        while i is not None and not seen[i]:
            seen[i] = True
            segs.append(i)
            i = by_from.get(et[i])
        return segs
    for i in range(n):
        if ef[i] not in targets:
            out.append((follow(i), False))
    for i in range(n):
        if not seen[i]:
            out.append((follow(i), True))
    return out


def pieces(count, e_from, e_to, pts, ny, nx, ycoord, xcoord, periodic=False, period=0.0, radius=0.0, fsum=math.fsum, walker=walk):
    """-> per range (table, length_terms, area_terms): `table` a structured array (DTYPE) sorted by first_edge, the two lists
    hold, piece by piece in the table's order, the float64 terms of that piece's two sums (before the radius; the area terms of an
    open piece too, though its area is NaN)"""
    count = np.asarray(count).astype(np.int64).ravel()
    e_from, e_to = np.asarray(e_from, dtype=np.int64), np.asarray(e_to, dtype=np.int64)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 4)
    assert e_from.size == e_to.size == pts.shape[0] == int(count.sum())
    latlon = radius > 0.0
    y, xe = np.asarray(ycoord, dtype=np.float64), x_nodes(xcoord, periodic, period)
    assert y.size == ny and xe.size == nx + (1 if periodic else 0)
    Y1, Y2 = interp_nodes(pts[:, 0], y), interp_nodes(pts[:, 2], y)
    X1, X2 = interp_nodes(pts[:, 1], xe), interp_nodes(pts[:, 3], xe)
    dX = X1 - X2
    with np.errstate(all='ignore'):
        ln = CR.haversine(X1, Y1, X2, Y2) if latlon else np.hypot(dX, Y1 - Y2)
        ya, yb = (np.sin(Y1), np.sin(Y2)) if latlon else (Y1, Y2)
        at = 0.5 * ((ya + yb) * dX)
    differ = ~((pts[:, 0] == pts[:, 2]) & (pts[:, 1] == pts[:, 3]))
    out, s0 = [], 0
    for c in count:
        sl = slice(s0, s0 + int(c))
        rows = []
        for segs, closed in walker(e_from[sl], e_to[sl], 2 * ny * nx):
            g = s0 + np.asarray(segs, dtype=np.int64)
            lt, art = ln[g][differ[g]], at[g]
            length, S = fsum(lt), fsum(art)
            if latlon:
                length, S = length * radius, S * (radius * radius)
            w = int((pts[g, 3] == nx).sum()) - int((pts[g, 1] == nx).sum()) if closed and periodic else 0
            rr = pts[g][:, [0, 2]]
            rows.append(((int(e_from[g].min()), g.size, bool(closed), w, length, S if closed else np.nan, float(rr.min()),
                          float(rr.max())), lt, art))
        rows.sort(key=lambda t: t[0][0])
        out.append((np.array([r[0] for r in rows], dtype=DTYPE), [r[1] for r in rows], [r[2] for r in rows]))
        s0 += int(c)
    return out


# ------------------------------------------------------------------ the windows of the two fixed-point sums
WINDOW_BITS = 160                       # five 32-bit limbs


def window_top(bound):
    """the exponent of a window's top from the bound on one term: frexp exponent + 12, never below -800; the window holds the bits
    2^(top - 160) ... 2^(top - 1)"""
    if not bound >= 2.0 ** -1022:
        return -800
    return max(math.frexp(bound)[1] + 12, -800)


def window(ycoord, xcoord, periodic=False, period=0.0, radius=0.0):
    """-> dict(length_top, length_bottom, area_top, area_bottom): a term t is added whole when its bits lie in
    [2^bottom, 2^top); bits under 2^bottom are cut off (toward zero), a term of 2^top or more makes the sum NaN.
    Bounds: length 1.0000001 * hypot(max |dx|, max |dy|) (3.2 on the sphere); area 1.0000001 * max |Y'| * max |dx| (max |Y'| = 1
    on the sphere); the seam cell is among the dx of a periodic plane."""
    y, xe = np.asarray(ycoord, dtype=np.float64), x_nodes(xcoord, periodic, period)
    mx = float(np.max(np.abs(np.diff(xe)))) if xe.size > 1 else 0.0
    dy = float(np.max(np.abs(np.diff(y)))) if y.size > 1 else 0.0
    my = float(np.max(np.abs(y)))
    if radius > 0.0:
        lb, ab = 3.2, 1.0000001 * 1.0 * mx
    else:
        lb, ab = 1.0000001 * float(np.hypot(mx, dy)), 1.0000001 * my * mx
    lt, at = window_top(lb), window_top(ab)
    return dict(length_top=lt, length_bottom=lt - WINDOW_BITS, area_top=at, area_bottom=at - WINDOW_BITS)


def cut(t, bottom):
    """the float64 t with its bits under 2^bottom dropped (toward zero): what a window with that bottom keeps of it"""
    t = float(t)
    if t == 0.0 or not math.isfinite(t):
        return t
    m, e = math.frexp(abs(t))
    M, sh = int(math.ldexp(m, 53)), (e - 53) - bottom                       # |t| = M 2^(e - 53)
    if sh >= 0:
        return t
    return math.copysign(math.ldexp(M >> -sh, bottom), t)


# ------------------------------------------------------------------ the limb model of the fixed-point sums, sound and broken
def round_exact(fr, ties_away=False):
    """a Fraction -> the nearest float64, half to even (ties_away True: half away from zero; None: half toward zero)"""
    if fr == 0:
        return 0.0
    neg, fr = fr < 0, abs(fr)
    e = fr.numerator.bit_length() - fr.denominator.bit_length()
    while Fraction(2) ** e > fr:
        e -= 1
    while Fraction(2) ** (e + 1) <= fr:
        e += 1
    scaled = fr / Fraction(2) ** (e - 52)                                   # in [2^52, 2^53)
    n, rem = divmod(scaled.numerator, scaled.denominator)
    twice = 2 * rem
    if twice > scaled.denominator or (twice == scaled.denominator and ties_away is not None and (ties_away or n & 1)):
        n += 1
    out = math.ldexp(float(n), e - 52)
    return -out if neg else out


def limb_sum(terms, top, defect=None):
    """The mechanism the header names, in Python integers: a window of five 32-bit limbs under 2^top kept in 64-bit words; a term
    cut at the limb boundaries into three chunks below 2^32, negated for a negative term; the words carried; a negative total
    complemented with borrows; the top 64 bits rounded half to even with a sticky bit for the rest.  `defect` breaks one step."""
    M32, W = (1 << 32) - 1, 1 << 64
    acc = [0] * 5
    for v in terms:
        v = float(v)
        if v == 0.0:
            continue
        m, e = math.frexp(abs(v))
        M, sh = int(math.ldexp(m, 53)), (e - 53) - (top - 160)
        if sh < 0:
            M, sh = (M >> -sh if -sh < 53 else 0), 0
        k, s = divmod(sh, 32)
        big = M << s
        for t, c in enumerate((big & M32, (big >> 32) & M32, big >> 64)):
            j = 4 - k - t
            if defect == 'a chunk one limb off at shift 17' and s == 17 and t == 1:
                j += 1
            if c:
                assert 0 <= j < 5
                acc[j] = (acc[j] + (-c if v < 0 else c)) % W
    w = [a - W if a >= W // 2 else a for a in acc]
    for j in range(4, 0, -1):
        c = w[j] >> 32
        w[j] -= c << 32
        if not (defect == 'a carry lost between limbs' and j == 2):
            w[j - 1] += c
    neg = w[0] < 0
    if neg:
        borrow = 0
        for j in range(4, -1, -1):
            t = -w[j] - borrow
            borrow = 0
            if j > 0 and t < 0:
                t += 1 << 32
                borrow = 0 if defect == 'no borrow on a negative sum' else 1
            w[j] = t
    total = sum(w[j] << (32 * (4 - j)) for j in range(5))
    if total == 0:
        return 0.0
    nb, e = total.bit_length(), top - 160
    if nb > 64 and defect == 'no sticky bit':
        total, e = total >> (nb - 64), e + nb - 64
    out = round_exact(Fraction(total) * Fraction(2) ** e, ties_away={'ties away from zero': True, 'ties toward zero': None}.get(defect, False))
    return -out if neg else out


DEFECTS = ('ties away from zero', 'ties toward zero', 'no sticky bit', 'a carry lost between limbs', 'no borrow on a negative sum',
           'a chunk one limb off at shift 17')


# ------------------------------------------------------------------ builders: topologies
def chain(ids, closed, tail=None):
    """the (e_from, e_to) of one chain in walk order from the ids of its segments: segment i starts on ids[i] and ends on
    ids[i + 1]; a ring's last segment ends on ids[0], an open chain's on `tail` (an id that is no segment's e_from)"""
    ids = np.asarray(ids, dtype=np.int64)
    assert closed or tail is not None
    return ids, np.concatenate([ids[1:], [ids[0] if closed else tail]]).astype(np.int64)


def stride_order(n):
    """position p holds walk index (p s) mod n for an odd s near n / 2 that is coprime to n: neighbours in memory are half a
    chain apart in the walk"""
    s = max(1, n // 2) | 1
    while math.gcd(s, n) != 1:
        s += 2
    return (np.arange(n, dtype=np.int64) * s) % n


def storage_orders(n, rng):
    """the four storage orders of a chain of n segments: name -> the walk index stored at each position"""
    return {'walk': np.arange(n, dtype=np.int64), 'reversed': np.arange(n, dtype=np.int64)[::-1].copy(),
            'random': rng.permutation(n).astype(np.int64), 'stride': stride_order(n)}


def unit_pts(n, ny, nx, salt=0):
    """n axis-aligned unit segments (r, c) -> (r, c + 1) spread over the plane: on coordinates that are the indices every length
    term is 1 and every area term is -r, so the sums are small integers"""
    i = np.arange(n, dtype=np.int64) + salt
    r, c = (i % ny).astype(np.float64), ((i * 7) % (nx - 1)).astype(np.float64)
    return np.stack([r, c, r, c + 1.0], axis=1)


CHAIN_LENGTHS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097)


def one_chain_per_range(closed, ny=8, nx=300, seed=5):
    """Every chain length on either side of a power of two, of a wave and of a block, each one in the four storage orders with its
    smallest id at the head, in the middle and at the tail of the walk: one chain per range.
    -> (count, e_from, e_to, pts, expect) with expect[r] = (first_edge, nseg) of range r's only piece."""
    rng = np.random.default_rng(seed)
    E = 2 * ny * nx
    cnt, EF, ET, PT, expect = [], [], [], [], []
    for n in CHAIN_LENGTHS:
        if closed and n < 2:
            continue
        for where in sorted({0, n // 2, n - 1}):
            for name, order in storage_orders(n, rng).items():
                ids = np.sort(rng.choice(E, n + 1, replace=False))
                rest = rng.permutation(ids[1:])
                tail, rest = int(rest[0]), rest[1:]
                walk_ids = np.concatenate([rest[:where], ids[:1], rest[where:]])    # the smallest id at walk index `where`
                ef, et = chain(walk_ids, closed, tail)
                cnt.append(n); EF.append(ef[order]); ET.append(et[order]); PT.append(unit_pts(n, ny, nx, len(cnt))[order])
                expect.append((int(ids[0]), n))
    return np.array(cnt, dtype=np.uint64), np.concatenate(EF), np.concatenate(ET), np.concatenate(PT), expect


def pieces_of_sizes(sizes_closed, ids, tails, rng, ny, nx):
    """one range of many pieces: piece k has sizes_closed[k] = (n, closed); its ids come from `ids` in turn, the tails of the open
    ones from `tails` (disjoint from ids); the segments are interleaved in memory by a random permutation"""
    EF, ET, at, nt = [], [], 0, 0
    for n, closed in sizes_closed:
        ef, et = chain(ids[at:at + n], closed, None if closed else tails[nt])
        at, nt = at + n, nt + (0 if closed else 1)
        EF.append(ef); ET.append(et)
    ef, et = np.concatenate(EF), np.concatenate(ET)
    o = rng.permutation(ef.size)
    return ef[o], et[o], unit_pts(ef.size, ny, nx)[o]


def many_pieces(ny=8, nx=300, seed=6):
    """300 two-segment rings, 100 one-segment open pieces and 50 open chains of 3 to 9 segments in ONE range -> records, 450"""
    rng = np.random.default_rng(seed)
    sizes = [(2, True)] * 300 + [(1, False)] * 100 + [(int(n), False) for n in rng.integers(3, 10, 50)]
    sizes = [sizes[i] for i in rng.permutation(len(sizes))]
    nid = sum(n for n, _ in sizes)
    pool = rng.permutation(2 * ny * nx)
    ef, et, pts = pieces_of_sizes(sizes, pool[:nid], pool[nid:nid + 150], rng, ny, nx)
    return np.array([ef.size], dtype=np.uint64), ef, et, pts, len(sizes)


def short_ranges(counts, ny=8, nx=300, seed=7):
    """ranges of the given counts, every one cut into pieces of 1 to 7 segments (a range of 1000 or more: one ring), ALL ranges
    drawing the same edge ids in the same order: a link or a root that crossed a range boundary would merge pieces"""
    rng = np.random.default_rng(seed)
    pool = rng.permutation(2 * ny * nx)
    big = max(int(c) for c in counts)
    ids, tails = pool[:big], pool[big:]
    EF, ET, PT = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)], [np.zeros((0, 4))]
    for c in counts:
        c, sizes = int(c), []
        while c:
            n = c if c >= 1000 else min(c, int(rng.integers(1, 8)))
            sizes.append((n, bool(n >= 2 and rng.random() < 0.5)))
            c -= n
        if sizes:
            ef, et, pts = pieces_of_sizes(sizes, ids, tails, rng, ny, nx)
            EF.append(ef); ET.append(et); PT.append(pts)
    return np.array(counts, dtype=np.uint64), np.concatenate(EF), np.concatenate(ET), np.concatenate(PT)


# ------------------------------------------------------------------ builders: exact sums on a Cartesian plane
EXACT_Y = np.array([1.0, 0.5])          # row 0: an area term is +-width itself; row 1: half of it


def exact_plane(widths):
    """xcoord for cells of the given widths, each one reproduced EXACTLY by x[j + 1] - x[j]: np.cumsum of the steps
    w0, -w0, w1, -w1, ... -- every partial sum is w_k or 0, so every one is exact whatever the widths (running sums of
    positive widths alone cannot be: 1 + 2^-53 is no float64).  Cell 2k, between nodes 2k and 2k + 1, has width widths[k]; the
    cells between are the way back (the entry asks no order of the coordinates: it reads them cell by cell).  -> xcoord (2 n + 1,);
    asserts the exactness."""
    w = np.asarray(widths, dtype=np.float64)
    assert w.size and (w > 0).all() and np.isfinite(w).all()
    steps = np.empty(2 * w.size)
    steps[0::2], steps[1::2] = w, -w
    x = np.concatenate([[0.0], np.cumsum(steps)])
    assert (x[0::2] == 0.0).all() and np.array_equal(x[1::2], w)
    assert np.array_equal(x[1::2] - x[0:-1:2], w) and np.array_equal(x[0:-1:2] - x[1::2], -w)
    return x


def term_pts(k, sign, row=0):
    """the segment along `row` over cell 2k of an exact_plane: its length term is the cell's width w, its area term
    sign * EXACT_Y[row] * w (from the far node to the near one for +, the other way for -)"""
    a, b = (2.0 * k + 1.0, 2.0 * k) if sign > 0 else (2.0 * k, 2.0 * k + 1.0)
    return [float(row), a, float(row), b]


def exact_records(groups, rng=None, order=None):
    """One range on an exact_plane.  groups: a list of pieces, each a list of signed terms (a 0.0 stands for a segment whose end
    points coincide: it adds to neither sum).  Every piece is a ring; segment k of the flat list runs over cell 2k of the plane,
    so its area term is the signed term itself and its length term the term's magnitude.  Links are free: ids are handed out in
    turn.  order: a permutation of the flat list for the storage order (default: as given).
    -> dict(count, e_from, e_to, pts, ny, nx, ycoord, xcoord, terms=groups)"""
    flat = [float(t) for g in groups for t in g]
    mags = [abs(t) if t != 0.0 else 1.0 for t in flat]                      # a coincident-end segment sits on a cell of width 1
    x = exact_plane(mags)
    nx, ny = x.size, 2
    pts, EF, ET, k = [], [], [], 0
    for g in groups:
        ef, et = chain(np.arange(k, k + len(g), dtype=np.int64) * 2 + 1, True)
        EF.append(ef); ET.append(et)
        for t in g:
            pts.append(term_pts(k, 1 if t > 0 else -1) if t != 0.0 else [0.0, 2.0 * k, 0.0, 2.0 * k])
            k += 1
    ef, et, pts = np.concatenate(EF), np.concatenate(ET), np.array(pts, dtype=np.float64)
    if order is not None:
        ef, et, pts = ef[order], et[order], pts[order]
    return dict(count=np.array([len(flat)], dtype=np.uint64), e_from=ef, e_to=et, pts=pts, ny=ny, nx=nx, ycoord=EXACT_Y.copy(),
                xcoord=x, terms=[[float(t) for t in g] for g in groups])


def p2(k):
    return math.ldexp(1.0, k)


ONE_UP = 1.0 + p2(-52)                  # the float64 after 1


def exact_cases():
    """name -> (terms of one ring, the float64 their exact sum rounds to), every expected value written out"""
    absorb = [1.0] + [p2(-60)] * 4096                                       # a running sum that starts at 1 never leaves it
    cases = {
        'absorption': (absorb, 1.0 + p2(-48)),
        'tie to even, down': ([1.0, p2(-53)], 1.0),
        'tie to even, up': ([ONE_UP, p2(-53)], 1.0 + p2(-51)),
        'sticky lifts the tie': ([1.0, p2(-53), p2(-140)], ONE_UP),
        'sticky pulls the tie down': ([ONE_UP, p2(-53), -p2(-140)], ONE_UP),
        'negative tie to even': ([-1.0, -p2(-53)], -1.0),
        'negative sticky': ([-1.0, -p2(-53), -p2(-140)], -ONE_UP),
        'cancellation': ([1.0, -1.0, p2(-80)], p2(-80)),
        'all limbs negative': ([-1.0, -p2(-70)], -1.0),
        'borrow through three limbs': ([1.0, -p2(-70)], 1.0),
        'borrow, exact': ([1.0, -p2(-53)], 1.0 - p2(-53)),
        'borrow, tie to even': ([1.0, -p2(-54)], 1.0),
        'borrow, sticky': ([1.0, -p2(-54), -p2(-140)], 1.0 - p2(-53)),
        'negative borrow': ([-1.0, p2(-70), -p2(-53)], -1.0),
        'cancels to +0': ([1.0, p2(-60), -1.0, -p2(-60), p2(-100), -p2(-100)], 0.0),
    }
    return cases


def every_shift_terms():
    """(1 + 2^-52) 2^-k for k = 0..95: first and last bit set, at every shift 0..31 against the limb grid and in every limb"""
    return [math.ldexp(ONE_UP, -k) for k in range(96)]


def bottom_terms(bottom):
    """-> (straddling, whole): `straddling` = one 53-bit term whose low 32 bits lie under 2^bottom and are cut off there, beside
    the window's last bit itself, in a sum small enough to show the cut; `whole` = one term whose last bit is the window's last"""
    return [math.ldexp(ONE_UP, bottom + 20), math.ldexp(1.0, bottom)], [math.ldexp(ONE_UP, bottom + 52)]


def all_ones_terms():
    """(1 - 2^-53) 2^-k for k = 0..94: all 53 bits set, so every one of the three chunks a term is cut into is non-zero -- the
    terms of every_shift_terms have an empty middle chunk -- at every shift 0..31 again, down to the window's last bit"""
    return [math.ldexp(1.0 - p2(-53), -k) for k in range(95)]


def random_terms(n=3000, seed=9):
    """n signed terms with random 53-bit mantissas (first and last bit set) and exponents in [-90, 0]"""
    rng = np.random.default_rng(seed)
    m = (rng.integers(0, 1 << 51, n, dtype=np.int64) << 1) | (1 << 52) | 1
    t = np.ldexp(m.astype(np.float64), rng.integers(-90, 1, n) - 52)
    t[0] = math.ldexp(float(m[0]), -52)                                      # the largest width: exponent 0
    return (t * rng.choice([-1.0, 1.0], n)).tolist()
