"""numpy restatement of the contour-length rule of K10 (xc_clen.hip) -- a helper for the tests, no tests here.

skimage's find_contours(image, level) with its defaults, restated (build-defined: skimage is not a dependency):
float64 arithmetic; a cell with a NaN corner emits nothing; case = (ul>c) + 2 (ur>c) + 4 (ll>c) + 8 (lr>c), 0 and 15
emit nothing; frac(a, b) = 0 if a == b else (c - a) / (b - a); edge points top (r0, c0 + frac(ul, ur)), bottom
(r0+1, c0 + frac(ll, lr)), left (r0 + frac(ul, ll), c0), right (r0 + frac(ur, lr), c0+1); saddles 6 and 9 pair like
fully_connected='low'; a segment with two equal end points is dropped.  End points map through np.interp onto the
coordinates; lengths are haversine (reference utils.__geodist) or hypot; a total of 0 is NaN (utils.py:603-604).
"""
import numpy as np

RADIUS = 6371200.0

T, B, L, R = 0, 1, 2, 3
# case -> the segments' end point ids (skimage _get_contour_segments, fully_connected='low')
PAIRS = {1: [(T, L)], 2: [(R, T)], 3: [(R, L)], 4: [(L, B)], 5: [(T, B)], 6: [(R, T), (L, B)], 7: [(R, B)],
         8: [(B, R)], 9: [(T, L), (B, R)], 10: [(B, T)], 11: [(B, L)], 12: [(L, R)], 13: [(T, R)], 14: [(L, T)]}
PAIRS_HIGH = dict(PAIRS)
PAIRS_HIGH.update({6: [(L, T), (R, B)], 9: [(T, R), (B, L)]})


def _frac(a, b, c):
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(a == b, 0.0, (c - a) / np.where(a == b, 1.0, b - a))


def segments(q, c, pairs=PAIRS):
    """index-space segments of level c on the 2-D field q: (r1, c1, r2, c2) arrays, degenerate ones dropped"""
    q = np.asarray(q, dtype=np.float64)
    c = float(c)
    ul, ur, ll, lr = q[:-1, :-1], q[:-1, 1:], q[1:, :-1], q[1:, 1:]
    with np.errstate(invalid='ignore'):
        mn = np.fmin(np.fmin(ul, ur), np.fmin(ll, lr))
        mx = np.fmax(np.fmax(ul, ur), np.fmax(ll, lr))
        sel = (mn <= c) & (c < mx) & ~(np.isnan(ul) | np.isnan(ur) | np.isnan(ll) | np.isnan(lr))
    r0, c0 = np.nonzero(sel)
    a, b, d, e = ul[sel], ur[sel], ll[sel], lr[sel]
    case = (a > c) * 1 + (b > c) * 2 + (d > c) * 4 + (e > c) * 8
    r0f, c0f = r0.astype(np.float64), c0.astype(np.float64)
    pts = {T: (r0f, c0f + _frac(a, b, c)), B: (r0f + 1.0, c0f + _frac(d, e, c)),
           L: (r0f + _frac(a, d, c), c0f), R: (r0f + _frac(b, e, c), c0f + 1.0)}
    out = [[], [], [], []]
    for cs, prs in pairs.items():
        m = case == cs
        if not m.any():
            continue
        for p, s in prs:
            out[0].append(pts[p][0][m]); out[1].append(pts[p][1][m])
            out[2].append(pts[s][0][m]); out[3].append(pts[s][1][m])
    if not out[0]:
        return tuple(np.zeros(0) for _ in range(4))
    r1, c1, r2, c2 = (np.concatenate(v) for v in out)
    keep = ~((r1 == r2) & (c1 == c2))
    return r1[keep], c1[keep], r2[keep], c2[keep]


def haversine(x1, y1, x2, y2):
    """utils.__geodist, in its operation order (radians; unit sphere)"""
    dlon = x2 - x1
    dlat = y2 - y1
    a = np.sin(dlat / 2.0) ** 2.0 + np.cos(y1) * np.cos(y2) * np.sin(dlon / 2) ** 2.0
    return 2.0 * np.arcsin(np.sqrt(a))


def segment_lengths(q, c, ycoord, xcoord, latlon, pairs=PAIRS):
    r1, c1, r2, c2 = segments(q, c, pairs)
    yi, xi = np.arange(len(ycoord)), np.arange(len(xcoord))
    y1, y2 = np.interp(r1, yi, ycoord), np.interp(r2, yi, ycoord)
    x1, x2 = np.interp(c1, xi, xcoord), np.interp(c2, xi, xcoord)
    return haversine(x1, y1, x2, y2) if latlon else np.hypot(x1 - x2, y1 - y2)


def contour_lengths(q2d, levels, ycoord, xcoord, latlon=False, pairs=PAIRS):
    """-> (totals f64 (N,), segment counts int64 (N,)) for one slab; ycoord / xcoord: float64 coordinate arrays (radians when
    latlon), i.e. what the library receives"""
    tot = np.empty(len(levels)); cnt = np.zeros(len(levels), dtype=np.int64)
    for k, c in enumerate(levels):
        if np.isnan(c):
            tot[k] = np.nan
            continue
        s = segment_lengths(q2d, c, ycoord, xcoord, latlon, pairs)
        cnt[k] = s.size
        t = float(np.sum(s))
        tot[k] = np.nan if t == 0 else (t * RADIUS if latlon else t)
    return tot, cnt


def plane_coords(ycoord, xcoord, latlon):
    """the float64 coordinate arrays the facade builds (reference core.py:1003-1004: float32 first, then radians in float32)"""
    y, x = np.asarray(ycoord).astype(np.float32), np.asarray(xcoord).astype(np.float32)
    if latlon:
        y, x = np.deg2rad(y), np.deg2rad(x)
    return y.astype(np.float64), x.astype(np.float64)


# ---- the same rule for every level at once (the GPU tests and tools/gpu_fuzz.py need it fast)
def segments_fast(q2d, levels, ycoord, xcoord, latlon=False, pairs=PAIRS, chunk=1 << 21):
    """Every segment of every level in one vectorised pass: for each NaN-free cell the crossed levels, mn <= c < mx, are the
    index range between two searchsorted lower bounds (what K10 computes), and every (cell, level) pair emits its segments at
    once.  Levels in any order; a NaN level crosses nothing.  -> (k level index, r1, c1, r2, c2, length) arrays, degenerate
    segments dropped.  `chunk`: (cell, level) pairs per step (bounds the memory)."""
    q = np.asarray(q2d, dtype=np.float64)
    lv = np.asarray(levels, dtype=np.float64)
    srt = np.where(np.isnan(lv), np.inf, lv)
    order = np.argsort(srt, kind='stable')
    ls = srt[order]
    ny, nx = q.shape
    yi, xi = np.arange(ny), np.arange(nx)
    ul, ur, ll, lr = (a.ravel() for a in (q[:-1, :-1], q[:-1, 1:], q[1:, :-1], q[1:, 1:]))
    with np.errstate(invalid='ignore'):
        ok = ~(np.isnan(ul) | np.isnan(ur) | np.isnan(ll) | np.isnan(lr))
    cell = np.nonzero(ok)[0]
    mn = np.fmin(np.fmin(ul[cell], ur[cell]), np.fmin(ll[cell], lr[cell]))
    mx = np.fmax(np.fmax(ul[cell], ur[cell]), np.fmax(ll[cell], lr[cell]))
    klo, khi = np.searchsorted(ls, mn, 'left'), np.searchsorted(ls, mx, 'left')
    n = np.maximum(khi - klo, 0)
    cell, klo, n = cell[n > 0], klo[n > 0], n[n > 0]
    ends = np.cumsum(n)
    out = [[] for _ in range(6)]
    i0 = 0
    while i0 < cell.size:                                   # whole cells per step, about `chunk` pairs each
        i1 = max(int(np.searchsorted(ends, (ends[i0 - 1] if i0 else 0) + chunk, 'right')), i0 + 1)
        cc, kl, nn = cell[i0:i1], klo[i0:i1], n[i0:i1]
        rep = np.repeat(np.arange(cc.size), nn)
        ks = kl[rep] + (np.arange(rep.size) - np.repeat(np.cumsum(nn) - nn, nn))
        ci = cc[rep]
        c = ls[ks]
        a, b, d, e = ul[ci], ur[ci], ll[ci], lr[ci]
        r0f, c0f = (ci // (nx - 1)).astype(np.float64), (ci % (nx - 1)).astype(np.float64)
        case = (a > c) * 1 + (b > c) * 2 + (d > c) * 4 + (e > c) * 8
        pts = {T: (r0f, c0f + _frac(a, b, c)), B: (r0f + 1.0, c0f + _frac(d, e, c)),
               L: (r0f + _frac(a, d, c), c0f), R: (r0f + _frac(b, e, c), c0f + 1.0)}
        for cs, prs in pairs.items():
            m = case == cs
            if not m.any():
                continue
            for p, s in prs:
                r1, c1, r2, c2 = pts[p][0][m], pts[p][1][m], pts[s][0][m], pts[s][1][m]
                keep = ~((r1 == r2) & (c1 == c2))
                r1, c1, r2, c2 = r1[keep], c1[keep], r2[keep], c2[keep]
                y1, y2 = np.interp(r1, yi, ycoord), np.interp(r2, yi, ycoord)
                x1, x2 = np.interp(c1, xi, xcoord), np.interp(c2, xi, xcoord)
                ln = haversine(x1, y1, x2, y2) if latlon else np.hypot(x1 - x2, y1 - y2)
                for o, v in zip(out, (order[ks[m][keep]], r1, c1, r2, c2, ln)):
                    o.append(v)
        i0 = i1
    if not out[0]:
        return (np.zeros(0, dtype=np.int64),) + tuple(np.zeros(0) for _ in range(5))
    return tuple(np.concatenate(o) for o in out)


def contour_lengths_fast(q2d, levels, ycoord, xcoord, latlon=False, pairs=PAIRS):
    """contour_lengths from segments_fast: the same counts and segment lengths, summed per level in another order"""
    N = len(levels)
    k, *_, ln = segments_fast(q2d, levels, ycoord, xcoord, latlon, pairs)
    cnt = np.bincount(k, minlength=N).astype(np.int64)
    t = np.bincount(k, weights=ln, minlength=N)
    tot = np.where(t == 0, np.nan, t * RADIUS if latlon else t)
    tot[np.isnan(np.asarray(levels, dtype=np.float64))] = np.nan
    return tot, cnt


def clen_bound(ycoord, xcoord, latlon):
    """K10's bound on one segment (k_clen_window): 3.2 on the unit sphere, else 1.0000001 x the largest cell diagonal"""
    if latlon:
        return 3.2
    my = float(np.max(np.abs(np.diff(ycoord)))) if len(ycoord) > 1 else 0.0
    mx = float(np.max(np.abs(np.diff(xcoord)))) if len(xcoord) > 1 else 0.0
    return 1.0000001 * float(np.hypot(mx, my))


def det_totals(q2d, levels, ycoord, xcoord, latlon=False):
    """K10's sum, modelled: the restatement's segment lengths through the oracle's fixed-point rule (deterministic_bin_sums) on
    the window of clen_bound, times the radius on the sphere, NaN for a total of 0 -> totals f64 (N,).  Levels ascending."""
    import xcontour_oracle as O
    N = len(levels)
    k, *_, ln = segments_fast(q2d, levels, ycoord, xcoord, latlon)
    t = O.deterministic_bin_sums(k + 1, ln, N, top=O.det_window_top(clen_bound(ycoord, xcoord, latlon)), nlimb=4)
    with np.errstate(invalid='ignore'):
        return np.where(t == 0, np.nan, t * RADIUS if latlon else t)


def launch_geometry(N, ny, nx, nslab, words=5, copy_cells=32767, wrap=False):
    """the launch choices of the tile-walk contour kernels, restated: K10 (launch_contour_lengths: words = 5 LDS words per (level,
    copy), copy_cells = 32767 cells per copy) and K15 (launch_contour_line_integrals: 10 words, 16383 cells).  LDS: the level values
    (+ 2 sentinels) 8 B each, per (level, copy) `words` x 8 B + a 4 B count, 16 B of slack, 48 KiB in all: as many copies (8, 4, 2, 1)
    as take every level, else one copy and level groups of G.  Tiles of 32 x 252 cells (wrap: the ring has nx cell columns); a block
    gives a copy 32 x 256 / ncopy cell slots per tile, so it may walk copy_cells x ncopy // 8192 tiles.  Blocks per slab: 2048 // nslab
    ('share'), at least 8 ('floor'), at least ntile / max_tiles ('capacity'), at most ntile ('ntile')"""
    lds_of = lambda g, nc: (g + 2) * 8 + g * nc * (words * 8 + 4) + 16
    ncopy = 8
    while ncopy > 1 and lds_of(N, ncopy) > 48 * 1024:
        ncopy //= 2
    G = N if lds_of(N, ncopy) <= 48 * 1024 else (48 * 1024 - 32) // (8 + words * 8 + 4)
    ncx = nx if wrap else nx - 1
    ntj = -(-(ny - 1) // 32) if ny > 1 else 0
    nti = -(-ncx // 252) if ncx > 0 else 0
    ntile = ntj * nti
    max_tiles = copy_cells * ncopy // (32 * 256)
    bps, rule = 0, None
    if ntile > 0:
        bps, rule = 2048 // nslab, 'share'
        if bps < 8:
            bps, rule = 8, 'floor'
        need = -(-ntile // max_tiles)
        if bps < need:
            bps, rule = need, 'capacity'
        if bps > ntile:
            bps, rule = ntile, 'ntile'
    return dict(N=N, ncopy=ncopy, G=G, ngroup=-(-N // G), ntile=ntile, bps=bps, bps_rule=rule, nslab=nslab)


def hashed_coords(n, salt=0, start=0.0, scale=1.0, descending=False):
    """n coordinates whose spacings scale (1 + 0.25 f(i)) differ in every cell (f hashed into [-1, 1), as in
    test_gpu_hist_variants.hashed); descending=True runs them from the top down"""
    i = np.arange(max(n - 1, 0), dtype=np.uint64)
    h = (i * np.uint64(40503) + np.uint64(salt) * np.uint64(97) + np.uint64(12345)) * np.uint64(2246822519)
    h = (h ^ (h >> np.uint64(13))) & np.uint64(0xffffffff)
    d = scale * (1.0 + 0.25 * (h.astype(np.float64) / 2.0 ** 31 - 1.0))
    c = start + np.concatenate([[0.0], np.cumsum(d)])
    return c[::-1].copy() if descending else c


def few_bits(n, salt, scale, bits_=20):
    """spacings scale (1 + 0.25 f(i)) cut to `bits_` significant bits; coordinates their exact running sum"""
    d = np.diff(hashed_coords(n, salt))
    e = np.floor(np.log2(d))
    d = np.floor(d * 2.0 ** (bits_ - 1 - e)) / 2.0 ** (bits_ - 1 - e) * scale
    return np.concatenate([[0.0], np.cumsum(d)])
