"""numpy / Python restatement of what K7's plan decides -- for the band walk, with the band a wave of k_lwa_strip walks, and for the
interval kernel (fast_plan: the CG ladder, the virtual blocks, and the column groups every persistent workgroup visits) -- a helper for
the tests, no tests here.

Which staging chunk a call of k_lwa_strip took, or how many target rows a thread of k_lwa held, cannot be seen from outside the library:
this restatement is the only witness, so test_lwa_plan_host.py pins it on a table worked out by hand from the LDS layout.

Restated: lwa_strip_lds (xc_lwa_walk.h:241-255), the band-walk half of lwa_plan (xc_lwa.hip:86-110), and lwa_row_needed / lwa_span_add
(xc_lwa_walk.h:35-52) as k_lwa_strip uses them (xc_lwa_walk.h:294-320) -- the calls that take the band walk: planes of up to 512
rows, or exact=True.  And, for the calls that take the interval kernel, fast_plan: the interval half of lwa_plan (xc_lwa.hip:63-85),
lwa_fast_lds (xc_lwa_fast.h:55-70), the XCD group order (xc_lwa_fast.h:98-105) and the persistent loop with its surplus skips
(xc_lwa_fast.h:137-144); test_lwa_fast_host.py pins it on a hand-worked table.  Which plane takes the interval kernel (`want_fast`,
xc_lwa.hip:68: the mode and the knobs) is not restated: the GPU tests ask ctx.last_lwa_path().
"""
import numpy as np

LDS_BUDGET = 150 * 1024   # kLdsBudget (xc_internal.h:147-151): XC_LDS_BUDGET_KB = 150
LWA_SW = 8                # xc_lwa_walk.h:6: waves per workgroup of k_lwa_strip = target rows per workgroup
LANES = 64                # columns of a strip: one per lane of a wave
WCHUNKS = (64, 32, 16)    # xc_lwa.hip:88: staging chunks, in the order they are tried
JT_SWITCH = 2.0e8         # xc_lwa.hip:107: ny^2 nx nslab from which a thread of k_lwa holds four target rows
LWA_NB = 4096             # xc_lwa_fast.h:52: value buckets of the interval kernel's bracket table
FAST_THREADS = 1024       # xc_lwa.hip:142: threads per workgroup of k_lwa_fast
FAST_CPT = 8              # xc_lwa_fast.h:108: cells per thread and round of loads


def strip_lds_bytes(ny, tsize, wplane, mplane, wchunk):
    """lwa_strip_lds(...).bytes (xc_lwa_walk.h:249-253): six [ny] double arrays (coord, Q, min, max, row weight, row metric), a
    [wchunk][64] double array per staged plane, 64 bytes for the union band, the [ny][65] strip of the tracer; rounded up to 16"""
    off = 6 * ny * 8
    off += (wchunk * LANES * 8 if wplane else 0) + (wchunk * LANES * 8 if mplane else 0)
    off += 64
    off += ny * 65 * tsize
    return (off + 15) & ~15


def planes(dA_rank, M_rank):
    """-> (wplane, mplane) of xc_lwa.hip:87: an absent metric is dA itself (core.py:789), so it has dA's rank"""
    assert dA_rank in ('row', 'plane') and M_rank in (None, 'row', 'plane')
    return dA_rank == 'plane', (dA_rank if M_rank is None else M_rank) == 'plane'


def strip_chunk(ny, tsize, dA_rank, M_rank):
    """xc_lwa.hip:88-89: the first of 64, 32, 16 whose layout fits the budget, 0 when none does"""
    wpl, mpl = planes(dA_rank, M_rank)
    for c in WCHUNKS:
        if strip_lds_bytes(ny, tsize, wpl, mpl, c) <= LDS_BUDGET:
            return c
    return 0


def walk_plan(nslab, ny, nx, tsize, dA_rank, M_rank, cus=256, knob_strip=1):
    """the band walk of one call -> ('strip', wchunk): one launch of k_lwa_strip staging `wchunk` rows at a time (where neither the weight
    nor the metric is a plane nothing is staged and wchunk is the 64 tried first), or ('stream', JT): k_lwa_prep + k_lwa<.., JT>.
    dA_rank 'row' | 'plane', M_rank None | 'row' | 'plane'; knob_strip: XC_LWA_STRIP (0 never the strip kernel, 2 at any grid size)"""
    if cus <= 0:
        cus = 256                                                                   # xc_lwa.hip:67
    wchunk = strip_chunk(ny, tsize, dA_rank, M_rank)
    nstrip = (nx + 63) // 64                                                        # xc_lwa.hip:90
    jgroups = (ny + LWA_SW - 1) // LWA_SW                                           # xc_lwa.hip:91
    few = nstrip * nslab * jgroups <= 2 * cus or knob_strip > 1                     # xc_lwa.hip:95: the grid does not fill the chip twice
    if (wchunk and knob_strip and ny <= 0x7fff and nx <= 0x7fffffff // ny and few   # xc_lwa.hip:96
            and nstrip <= 0x7fffffff and jgroups <= 65535 and nslab <= 65535):
        return 'strip', wchunk
    if (nstrip + 63) // 64 > 65535:                                                 # xc_lwa.hip:106
        raise ValueError('xc_lwa: nx too large')
    return 'stream', (1 if float(ny) * float(ny) * float(nx) * float(nslab) < JT_SWITCH else 4)    # xc_lwa.hip:107


def largest_ny(target, nslab, nx, tsize, dA_rank, M_rank, **kw):
    """the largest ny for which walk_plan gives `target`: the tightest fit of that plan"""
    hit = [ny for ny in range(2, 600) if walk_plan(nslab, ny, nx, tsize, dA_rank, M_rank, **kw) == target]
    assert hit and hit[-1] < 599, target
    return hit[-1]


def smallest_stack(target, ny, nx, tsize, dA_rank, M_rank, **kw):
    """the smallest nslab for which walk_plan gives `target`"""
    for nslab in range(1, 65536):
        if walk_plan(nslab, ny, nx, tsize, dA_rank, M_rank, **kw) == target:
            return nslab
    raise AssertionError(target)


# ---------------------------------------------------------------- the band of one wave of k_lwa_strip
def lwa_keep(part, increase):
    """xc_lwa_walk.h:27: 0 both sides, 1 the near side only, -1 the far side only; part 0 'all', 1 'upper', 2 'lower'"""
    return 0 if part == 0 else (1 if (part == 1) == bool(increase) else -1)


def strip_extrema(q, strip):
    """xc_lwa_walk.h:294-303: the NaN-skipping min / max of every row of the 64-column strip (columns past the plane are NaN in LDS:
    skipped); a row without a number keeps +inf / -inf"""
    s = np.asarray(q, dtype=np.float64)[:, strip * LANES:(strip + 1) * LANES]
    return np.fmin.reduce(s, axis=1, initial=np.inf), np.fmax.reduce(s, axis=1, initial=-np.inf)


def row_needed(rmin, rmax, Qy, tlo, thi, near, inc_eff, keep, v2):
    """lwa_row_needed (xc_lwa_walk.h:35-42), elementwise"""
    anypos = (thi > Qy) if v2 else (rmax > thi)
    anyneg = (tlo < Qy) if v2 else (rmin < tlo)
    nd = np.where(near, anyneg if inc_eff else anypos, anypos if inc_eff else anyneg)
    return nd & ~((keep != 0) & ((keep > 0) != near))


def band(q, Q, coord, increase, part, variant, j, strip):
    """[y0, y1) of the rows the wave of target row j walks in 64-column strip `strip` (xc_lwa_walk.h:306-320): the first and one past
    the last row that lwa_row_needed lets through (lwa_span_add); an empty band is (ny, 0)"""
    Q, coord = np.asarray(Q, dtype=np.float64), np.asarray(coord, dtype=np.float64)
    ny = Q.size
    mn, mx = strip_extrema(q, strip)
    coord_incre = not (coord[-1] < coord[0])                                        # lwa_coord_incre, xc_lwa_walk.h:20
    inc_eff = (not increase) if variant else bool(increase)                         # xc_lwa_walk.h:307
    keep = lwa_keep(part, increase)
    tlo, thi = (mn[j], mx[j]) if variant else (Q[j], Q[j])                          # xc_lwa_walk.h:312
    near = (coord >= coord[j]) if coord_incre else (coord <= coord[j])              # lwa_near, xc_lwa_walk.h:23
    with np.errstate(invalid='ignore'):
        hit = np.flatnonzero(row_needed(mn, mx, Q, tlo, thi, near, inc_eff, keep, bool(variant)))
    return (int(hit[0]), int(hit[-1]) + 1) if hit.size else (ny, 0)


def bands(q, Q, coord, increase, part, variant, strip):
    """band for every target row of the strip at once (the same rule on a (target row, row) matrix) -> (y0[ny], y1[ny])"""
    Q, coord = np.asarray(Q, dtype=np.float64), np.asarray(coord, dtype=np.float64)
    ny = Q.size
    mn, mx = strip_extrema(q, strip)
    coord_incre = not (coord[-1] < coord[0])
    inc_eff = (not increase) if variant else bool(increase)
    tlo, thi = (mn, mx) if variant else (Q, Q)
    near = (coord[None, :] >= coord[:, None]) if coord_incre else (coord[None, :] <= coord[:, None])
    with np.errstate(invalid='ignore'):
        hit = row_needed(mn[None, :], mx[None, :], Q[None, :], tlo[:, None], thi[:, None], near, inc_eff, lwa_keep(part, increase),
                         bool(variant))
    some = hit.any(axis=1)
    return np.where(some, hit.argmax(axis=1), ny), np.where(some, ny - hit[:, ::-1].argmax(axis=1), 0)


def workgroups(y0, y1, wchunk):
    """what the workgroups of one strip (LWA_SW consecutive target rows each) stage, from their waves' bands -> a list of dicts:
    'union' (Y0, Y1) (xc_lwa_walk.h:326-333; (ny, 0) when every wave's band is empty), 'chunks' the number of trips of the chunk loop,
    'cut' a wave's band holds a chunk boundary, 'late' a wave's band starts in a chunk other than the first"""
    ny, out = len(y0), []
    for g in range(0, ny, LWA_SW):
        a, b = y0[g:g + LWA_SW], y1[g:g + LWA_SW]
        live = a < b
        Y0, Y1 = (int(a[live].min()), int(b[live].max())) if live.any() else (ny, 0)
        edges = np.arange(Y0 + wchunk, Y1, wchunk) if Y1 > Y0 else np.empty(0, dtype=np.int64)
        cut = any(((a[live][:, None] < edges[None, :]) & (edges[None, :] < b[live][:, None])).ravel())
        out.append({'union': (Y0, Y1), 'chunks': -(-(Y1 - Y0) // wchunk) if Y1 > Y0 else 0, 'cut': bool(cut),
                    'late': bool(live.any() and (a[live] >= Y0 + wchunk).any())})
    return out


# ---------------------------------------------------------------- the interval kernel
def fast_lds_bytes(ny, CG):
    """lwa_fast_lds(...).bytes (xc_lwa_fast.h:61-70): Q' [ny + 1] and the difference arrays D0, D1 [CG][ny + 1] in doubles, then the
    bucket table [LWA_NB + 1] in ints"""
    L = ny + 1
    return (L + 2 * CG * L) * 8 + (LWA_NB + 1) * 4


def fast_group_x0(vb, CG):
    """group_x0 (xc_lwa_fast.h:102-105): the first column of virtual block vb = 8 k + xcd -- the 16 / CG groups of a 16-column line stay
    on one XCD"""
    GQ = 16 // CG
    kq, xcd = vb >> 3, vb & 7
    return (((kq // GQ) * 8 + xcd) * GQ + kq % GQ) * CG


def fast_plan(nslab, ny, nx, cus=256):
    """the interval kernel of one call -> None where no rung of the CG ladder fits (or the plane has 2^29 cells or more:
    xc_lwa.hip:69), else a dict: 'CG' columns per workgroup, 'lds_bytes', 'nvb' virtual blocks, 'grid' (x, y), 'visits' -- for every
    block of grid x the (x0, ncol) of the column groups it runs, in order -- and 'skips' -- for every block the surplus virtual blocks it
    steps over, as ('entry' | 'mid', trip): on entry (xc_lwa_fast.h:138, before its first group) or in mid-loop (:144, behind one)"""
    if cus <= 0:
        cus = 256                                                                   # xc_lwa.hip:67
    CG = 0
    if ny * nx < (1 << 29):                                                         # xc_lwa.hip:69
        for c in (4, 2, 1):                                                         # xc_lwa.hip:70-71
            if not CG and fast_lds_bytes(ny, c) <= LDS_BUDGET:
                CG = c
    if not CG:
        return None
    ngrp, gq = (nx + CG - 1) // CG, 8 * (16 // CG)                                  # xc_lwa.hip:77
    nvb = ((ngrp + gq - 1) // gq) * gq                                              # xc_lwa.hip:78
    pw = max(8, (cus // 8) * 8)                                                     # xc_lwa.hip:81-82
    gx = min(nvb, pw)                                                               # xc_lwa.hip:83
    visits, skips = [], []
    for b in range(gx):
        v, sk = [], []
        for trip, vb in enumerate(range(b, nvb, gx)):                               # xc_lwa_fast.h:137-144, 236
            x0 = fast_group_x0(vb, CG)
            if x0 >= nx:
                sk.append(('mid' if v else 'entry', trip))
            else:
                v.append((x0, min(CG, nx - x0)))                                    # xc_lwa_fast.h:142
        visits.append(v)
        skips.append(sk)
    return {'CG': CG, 'lds_bytes': fast_lds_bytes(ny, CG), 'nvb': nvb, 'grid': (gx, nslab), 'visits': visits, 'skips': skips}


def fast_rounds(ny, CG):
    """-> (cells of a group, rounds of FAST_CPT * FAST_THREADS cells its search loop makes (xc_lwa_fast.h:147), the `split` of its
    prefix sums (xc_lwa_fast.h:203: 2 while four tasks per column fit the 16 waves))"""
    ncell = ny * CG
    return ncell, -(-ncell // (FAST_CPT * FAST_THREADS)), (2 if 4 * CG <= FAST_THREADS // 64 else 1)
