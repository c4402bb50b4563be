"""Planes on which every sum of K7's local wave activity is exact, a Python-integer model of the interval kernel's own chain, and the
oracle's loop body for sampled target rows -- helpers for test_lwa_fast_host.py and test_gpu_lwa_fast.py, no tests here.

Exactness.  Tracer cells and reference levels are integers or half-integers of magnitude <= ~2^11 (times one power of two, `scale`), the
weight dA an integer in [1, 256] with max 256 (so dA / max and dA * (1 / max) are the same exact number), the metric M an integer in
[1, 16] (or dA itself).  Every term (Q - q) (dA / 256) M, every partial sum of such terms in ANY order, the interval kernel's
(q' - c) W, its difference arrays, its prefix sums and its final (Q'_j - c) S0_j - S1_j are then integers in units of scale / 512 and
stay below 2^53 -- `build` asserts that with Python integers -- so the oracle (numpy's order), the band walk (the same order) and the
interval kernel (LDS atomics in arrival order, sums of pieces, a difference of two products) must give the SAME double: the comparison
is ==, and a mismatch is a wrong term, never rounding.

The model (`model`) is written from the header comment of xc_lwa_fast.h -- lower and upper bound of one search, near or far, the index p,
the four adds, the prefix sums in 128 pieces with the second half's base, the final form -- not from the oracle; `defect` swaps one step
for a wrong one (test_lwa_fast_host.py shows which cases notice).
"""
import bisect

import numpy as np

DT = {'f64': np.float64, 'f32': np.float32}
PARTS = (('all', 0), ('upper', 1), ('lower', 2))
RANKS = [(da, m) for da in ('row', 'plane') for m in (None, 'row', 'plane')]
QLIM = 512                # tracer cells of the random field: integers in [-QLIM, QLIM]
REF_END = 516             # the reference state ends at -516.5 and +516: a little past the tracer's range on both sides
PLANT = ('below', 'above', 'desc', 'plateau')
STATES = ('mixed', 'constant', 'two', 'lastbucket')
DEFECTS = ('a_for_b', 'b_for_a', 'a_lt_y', 'b_ge_y1', 'minus_at_y', 'no_half_base', 'side', 'm_rank')


def plateau_len(ny):
    """the long plateau of the 'mixed' reference state: 70 levels (more than a wave, more than one piece of the prefix sums up to
    8960 rows) where the plane has room for it beside the two end plateaus, a quarter of the levels otherwise"""
    return 70 if ny >= 280 else ny // 4


def _state(rng, ny, state):
    """Q' (non-decreasing) in half units (2 Q'), as int64"""
    lo, hi = -2 * REF_END - 1, 2 * REF_END                       # -516.5 (a half-integer), +516 (an integer)
    if state == 'constant':
        return np.full(ny, 6, dtype=np.int64)                       # 3 everywhere: no bucket width, and cells that tie with every level
    if state == 'two':
        return np.where(np.arange(ny) < ny // 3, -41, 62).astype(np.int64)
    if state == 'lastbucket':
        # Q'_0 = -2^20: a bucket is (2^20 + 516) / 4096 ~ 256 wide and the last one starts at ~260; every other level is in it, and the
        # cells above 260 meet the whole run of levels behind ONE table entry (the full binary search)
        Q2 = np.sort(rng.integers(2 * 262, hi + 1, ny))
        Q2[0], Q2[-1] = -2 ** 21, hi
        return Q2.astype(np.int64)
    assert state == 'mixed'
    Q2 = np.sort(rng.integers(lo, hi + 1, ny)).astype(np.int64)
    pe, pl = max(1, min(5, ny // 8)), plateau_len(ny)
    Q2[:pe], Q2[ny - pe:] = lo, hi                                  # a plateau at each end, past the tracer's range
    if pl >= 2:
        m0 = (ny - pl) // 2
        Q2[m0:m0 + pl] = (Q2[m0] // 2) * 2                          # the long one, on an INTEGER level: whole-plateau ties with cells
    return np.sort(Q2)


def plateau_level2(Q2):
    """2 x the INTEGER level with the longest run of equal levels (a cell can sit on it in either tracer type)"""
    v, n = np.unique(Q2[Q2 % 2 == 0], return_counts=True)
    return int(v[n.argmax()])


def build(ny, nx, dt='f64', increase=True, coord_up=True, da='plane', m='plane', seed=0, k=0, state='mixed', planted=(), nan=True,
          wseed=None):
    """-> dict.  For the library / the oracle: 'q' (ny, nx) of the dtype, 'Q' (ny,), 'coord' (ny,), 'dA' (ny,) or (ny, nx), 'M' the
    same or None, 'dA_max' 256.0, 'increase'.  For the model: 'q2' / 'Q2' = 2 q / 2 Q before scaling (int64; NaN cells in 'qnan'),
    'dAi' / 'Mi' the integer weights (NaN ones in 'dAnan' / 'Mnan'), 'scale' = 2^k.
    da 'row' | 'plane', m None | 'row' | 'plane'; state: see STATES; planted: ((x, kind), ...) with kind in PLANT; nan: NaN cells, one
    whole NaN column (planes of 3 columns or more) and NaN weights in plane-rank dA and M; wseed: the seed of the weights (slabs of a
    stack share them)."""
    assert ny >= 2 and nx >= 1 and state in STATES and (k == 0 or dt == 'f64')
    rng = np.random.default_rng([seed, ny, nx])
    wrng = np.random.default_rng([1000 + (seed if wseed is None else wseed), ny, nx])
    s = 1 if increase else -1
    Qp2 = _state(rng, ny, state)                                                      # 2 Q', non-decreasing
    assert (np.diff(Qp2) >= 0).all()
    # q' = s q: a meridional trend plus noise -- cells below and above their row's level, so both sides contribute
    trend = np.rint(np.linspace(-400, 400, ny)).astype(np.int64)
    qp = np.clip(trend[:, None] + rng.integers(-100, 101, (ny, nx)), -QLIM, QLIM)
    lvl2 = plateau_level2(Qp2)
    px = {}
    for x, kind in planted:
        assert 0 <= x < nx and kind in PLANT and x not in px
        px[x] = kind
        if kind == 'below':
            qp[:, x] = -(REF_END + 4) if state != 'lastbucket' else -2 ** 20 - 4       # below Q'_0
        elif kind == 'above':
            qp[:, x] = REF_END + 4                                                    # above Q'_last
        elif kind == 'desc':
            qp[:, x] = ny // 2 - np.arange(ny)                                        # strictly descending in y: every cell far from its own row
        else:
            qp[:, x] = lvl2 // 2                                                      # ON the plateau (an integer level in the 'mixed' state)
    q2 = 2 * s * qp                                                                   # int64; NaN cells in `qnan`
    qnan = np.zeros((ny, nx), dtype=bool)
    free = np.array([x not in px for x in range(nx)])
    if nan and ny * nx >= 8:
        n = max(1, ny * nx // 50)
        qnan[rng.integers(0, ny, n), rng.integers(0, nx, n)] = True
        if nx >= 3 and free.any():
            qnan[:, min(np.flatnonzero(free), key=lambda x: abs(x - nx // 2))] = True  # one whole NaN column
        qnan[:, ~free] = False                                                        # planted columns keep every cell
    Q2 = s * Qp2

    def weights(rank, top, pin):
        if rank is None:
            return None, None
        w = wrng.integers(1, top + 1, ny if rank == 'row' else (ny, nx))
        bad = np.zeros(w.shape, dtype=bool)
        if pin:
            w[(ny // 3,) if rank == 'row' else (ny // 3, 0)] = top                    # nanmax = 256 = 2^8 exactly
        if nan and rank == 'plane' and ny * nx >= 8:
            bad[wrng.integers(0, ny, 3), wrng.integers(0, nx, 3)] = True
            if pin:
                bad[ny // 3, 0] = False
        return w, bad
    (dAi, dAnan), (Mi, Mnan) = weights(da, 256, True), weights(m, 16, False)

    def f(a, bad, dtype, mul=1.0):
        return None if a is None else (np.where(bad, np.nan, a.astype(np.float64)) * mul).astype(dtype)
    scale = 2.0 ** k
    case = {'ny': ny, 'nx': nx, 'dt': dt, 'increase': bool(increase), 'da': da, 'm': m, 'k': k, 'scale': scale, 'state': state,
            'q2': q2, 'qnan': qnan, 'Q2': Q2, 'dAi': dAi, 'dAnan': dAnan, 'Mi': Mi, 'Mnan': Mnan, 'planted': dict(px),
            'q': f(q2, qnan, DT[dt], 0.5 * scale), 'Q': f(Q2, False, np.float64, 0.5 * scale), 'dA': f(dAi, dAnan, np.float64),
            'M': f(Mi, Mnan, np.float64), 'dA_max': 256.0, 'coord': np.linspace(-80, 80, ny) if coord_up else np.linspace(80, -80, ny)}
    # ---- the bound, with Python integers: in units of scale / 512 every term, every partial sum of terms of one column, the products
    # (Q'_j - c) S0_j and the sums S1_j are at most ny * max|2 (u - v)| * max(dA M) -- u, v any two of the cells and levels
    big = max(int(np.abs(Q2).max()), int(np.abs(q2).max()))
    wmax = int(dAi.max()) * int((dAi if Mi is None else Mi).max())
    check_bound(ny, big, wmax)
    assert float(np.nanmax(case['dA'])) == 256.0
    assert np.array_equal(case['q'].astype(np.float64), f(q2, qnan, np.float64, 0.5 * scale), equal_nan=True)    # the dtype holds every cell
    for a in (case['q'], case['Q'], case['dA'], case['M'], case['coord']):
        if a is not None:
            a.setflags(write=False)
    return case


def check_bound(ny, big, wmax):
    """ny terms of at most 2 big (twice a difference of two cells or levels, each at most big / 2) times wmax (dA M, 256 W): below 2^53
    in units of scale / 512 -- Python integers, no overflow to hide behind"""
    assert isinstance(ny, int) and isinstance(big, int) and isinstance(wmax, int)
    assert ny * (2 * big) * wmax < 2 ** 53, (ny, big, wmax)


def facts(case):
    """what a 'mixed' case was built to hold -> dict of booleans / counts, for the tests that stand on them"""
    s = 1 if case['increase'] else -1
    Qp2 = s * case['Q2']
    cells = s * case['q2'][~case['qnan']]
    v, n = np.unique(Qp2, return_counts=True)
    pe = 1
    while pe < len(Qp2) and Qp2[pe] == Qp2[0]:
        pe += 1
    return {'integers': bool((Qp2 % 2 == 0).any()), 'halves': bool((Qp2 % 2 != 0).any()), 'longest': int(n.max()),
            'first_run': pe, 'last_run': int((Qp2 == Qp2[-1]).sum()),
            'past_low': bool(Qp2[0] < cells.min()) if not case['planted'] else None,
            'past_high': bool(Qp2[-1] > cells.max()) if not case['planted'] else None,
            'ties': int(np.isin(cells, Qp2).sum()), 'nan_cells': int(case['qnan'].sum())}


# ---------------------------------------------------------------- the model
def lwa_keep(part, increase):
    """0 both sides, 1 the near side only, -1 the far side only (xc_lwa_walk.h: lwa_keep); part 0 'all', 1 'upper', 2 'lower'"""
    return 0 if part == 0 else (1 if (part == 1) == bool(increase) else -1)


def model_int(case, part, defect=None):
    """the chain of k_lwa_fast in Python integers -> [ny][nx] integers in units of scale / 512.  part 0 | 1 | 2."""
    assert defect is None or defect in DEFECTS
    ny, nx = case['ny'], case['nx']

    def ints(a, bad):                                              # Python integers, None for NaN
        return None if a is None else np.where(bad, None, a.astype(object))
    q2, dAi, Mi = ints(case['q2'], case['qnan']), ints(case['dAi'], case['dAnan']), ints(case['Mi'], case['Mnan'])
    s = 1 if case['increase'] else -1
    Qp = [s * int(v) for v in case['Q2']]                          # Q' = s Q, non-decreasing
    c = Qp[ny // 2]                                                # the reference level c
    keep = lwa_keep(part, case['increase'])
    side = 2 if keep < 0 else keep                                 # 0 both sides, 1 near, 2 far
    if defect == 'side':
        side = {0: 0, 1: 2, 2: 1}[side]
    da_row = case['da'] == 'row'
    Mp = dAi if Mi is None else Mi                                 # no M: the weight itself
    m_row = da_row if Mi is None else case['m'] == 'row'
    m_wrong = defect == 'm_rank' and Mi is None and da_row         # the rank of an absent M read as 'not a row': a plane index into the row
    per = -(-ny // 128)                                            # rows per piece: 2 waves x 64 lanes per array
    out = [[0] * nx for _ in range(ny)]
    for x in range(nx):
        D0, D1 = [0] * (ny + 1), [0] * (ny + 1)
        for y in range(ny):
            qc, w0 = q2[y, x], (dAi[y] if da_row else dAi[y, x])
            w1 = Mp[(y * nx + x) % ny] if m_wrong else (Mp[y] if m_row else Mp[y, x])
            if qc is None or w0 is None or w1 is None:
                continue                                            # NaN tracer / weight: nansum skips the term
            qv, W = s * int(qc), int(w0) * int(w1)                  # W in units of 1 / 256
            b = bisect.bisect_left(Qp, qv)                          # #{j: Q'_j <  q'}
            a = bisect.bisect_right(Qp, qv)                         # #{j: Q'_j <= q'}
            if defect == 'a_for_b':
                b = a
            if defect == 'b_for_a':
                a = b
            p = -1
            if (a < y) if defect == 'a_lt_y' else (a <= y):
                if side != 2:
                    p = a                                           # near-side term of targets [a, y]
            elif b >= y + (1 if defect == 'b_ge_y1' else 2):
                if side != 1:
                    p = b                                           # far-side term of targets [y + 1, b - 1]
            if p >= 0:
                e = y if defect == 'minus_at_y' else y + 1
                D0[p] += W; D0[e] -= W
                D1[p] += (qv - c) * W; D1[e] -= (qv - c) * W
        for D in (D0, D1):                                          # prefix sums in 128 pieces; the second wave starts from the first one's total
            tot = [sum(D[min(i * per, ny):min((i + 1) * per, ny)]) for i in range(128)]
            half = sum(tot[:64])
            for i in range(128):
                run = sum(tot[(i // 64) * 64:i]) + (half if i >= 64 and defect != 'no_half_base' else 0)
                for j in range(min(i * per, ny), min((i + 1) * per, ny)):
                    run += D[j]
                    D[j] = run
        for j in range(ny):
            out[j][x] = s * ((Qp[j] - c) * D0[j] - D1[j])
    return out


def model(case, part, defect=None):
    """model_int as doubles: |n| < 2^53 and scale / 512 is a power of two, so the conversion is exact"""
    r = model_int(case, part, defect)
    assert all(abs(v) < 2 ** 53 for row in r for v in row)
    return np.array([[float(v) for v in row] for row in r], dtype=np.float64).reshape(case['ny'], case['nx']) * (case['scale'] / 512.0)


# ---------------------------------------------------------------- the oracle's loop body, row by row
def lwa_rows(q, Q, coord, dA, rows, increase=True, part='all', metric=None):
    """core.py:752-791 for the target rows `rows` only (the oracle's own loop body, one j at a time: a full 1801-row plane has 1801
    of them at ~0.2 s each); dA (ny,) or (ny, nx), metric None (M = dA, core.py:789) or the same shapes"""
    q64 = np.asarray(q).astype(np.float64)
    dA2 = np.asarray(dA, dtype=np.float64)
    dA2 = dA2[:, None] if dA2.ndim == 1 else dA2
    wei = dA2 / np.nanmax(dA2)                                                         # core.py:723-724
    M = dA2 if metric is None else np.asarray(metric, dtype=np.float64)
    M = M[:, None] if M.ndim == 1 else M
    cinc = not (coord[-1] < coord[0])
    out = np.empty((len(rows), q64.shape[1]))
    for i, j in enumerate(rows):
        qe = q64 - Q[j]                                                               # core.py:754
        m = ((coord >= coord[j]) if cinc else (coord <= coord[j]))[:, None]
        if increase:                                                                   # core.py:759-766
            mask3 = np.where(np.logical_and(qe < 0, m), 1, np.where(m, 0, np.where(qe > 0, -1, 0)))
        else:
            mask3 = np.where(np.logical_and(qe > 0, m), 1, np.where(m, 0, np.where(qe < 0, -1, 0)))
        if part == 'all':                                                              # core.py:773-784
            mf = mask3.astype(np.float64)
        else:
            pos = (part == 'upper') == bool(increase)
            mf = np.where(mask3 > 0 if pos else mask3 < 0, mask3, np.nan)
        out[i] = -np.nansum(qe * mf * wei * M, axis=0)                                # core.py:789
    return out


def sample_rows(ny):
    """the target rows a tall plane is compared on: the first and last three, ny/2 - 1 .. ny/2 + 1 (the level c), and both sides of
    the piece edges per, 64 per, 64 per + per of the prefix sums (per = ceil(ny / 128))"""
    per = -(-ny // 128)
    rows = {0, 1, 2, ny - 3, ny - 2, ny - 1, ny // 2 - 1, ny // 2, ny // 2 + 1}
    for e in (per, 64 * per, 64 * per + per):
        rows |= {e - 2, e - 1, e, e + 1}
    return sorted(r for r in rows if 0 <= r < ny)
