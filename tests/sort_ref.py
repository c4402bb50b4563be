"""host-side reference of the K8 exact sort (xc_sort.hip) for tests/test_gpu_sort_limits.py -- a helper, no tests here.

The order is oracle.sorted_profile's: a stable ascending argsort of the valid cells (not NaN, mask == 1) in row-major order,
`-q` first where `negate`, float32 tracers compared after the exact widening to float64.

The exact permutation check: with the integer payload dA[i] = i + 1 (float64, flat cell index i) every partial sum of the device
scan is an integer below 2^53 (6.48 M cells: 2.1e13), so the scan is exact in any order of summation and
np.diff(acum[:n], prepend=0) - 1 IS the permutation the device applied -- every tie and every pair visible, no tolerance.
"""
import json
import os
import sys

import numpy as np

# ---- limits of the repair kernel, restated from xcontour_amd/csrc/xc_sort.hip ("constexpr int FIX_C = 1024, FIX_RUN = 128, ...",
# above k_fix_runs): a block owns the runs whose head lies in FIX_C consecutive sorted positions; a run that is out of order is
# repaired in LDS when it holds at most FIX_RUN cells.  read_fix_limits() reads the line itself: a change of either limit fails
# the tests that place runs on these edges instead of silently moving the edge.
FIX_C, FIX_RUN = 1024, 128
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read_fix_limits():
    import re
    with open(os.path.join(ROOT, 'xcontour_amd', 'csrc', 'xc_sort.hip')) as f:
        m = re.search(r'constexpr int FIX_C = (\d+), FIX_RUN = (\d+),', f.read())
    return int(m.group(1)), int(m.group(2))


def as_f64(q, negate=False):
    x = np.asarray(q).astype(np.float64).ravel()                 # exact for float32
    return -x if negate else x


def full_order(q, negate=False):
    """stable argsort of ALL non-NaN cells of one plane (flat cell indices)"""
    x = as_f64(q, negate)
    idx = np.flatnonzero(~np.isnan(x))
    return idx[np.argsort(x[idx], kind='stable')]


def valid_order(q, mask=None, negate=False, order=None):
    """(flat indices of the valid cells in sorted order, their values).  `order`: full_order(q, negate) computed before -- a
    stable sort of a subset is the stable sort of the whole with the other cells left out."""
    x = as_f64(q, negate)
    if order is None:
        order = full_order(q, negate)
    if mask is not None:
        order = order[np.asarray(mask).ravel()[order] == 1]
    return order, x[order]


def int_payload(ny, nx, slab=0):
    """dA[i] = i + 1 (+ slab * n: a per-slab payload names its slab)"""
    n = ny * nx
    return (np.arange(1, n + 1, dtype=np.float64) + float(slab * n)).reshape(ny, nx)


def applied_permutation(acum, m, slab=0, n=None):
    """the flat cell indices in the order the device put them, from the cumulative sum of the integer payload"""
    d = np.diff(np.asarray(acum[:m], dtype=np.float64), prepend=0.0) - 1.0 - (float(slab * n) if slab else 0.0)
    return d


def assert_permutation(r, q, mask=None, negate=False, order=None, slab=None, payload_slab=0, what=''):
    """nvalid, the exact permutation and the sorted values of one plane of a sort_profile result made with int_payload()"""
    n = np.asarray(q).size
    g = (lambda k: r[k]) if slab is None else (lambda k: r[k][slab])
    order, xs = valid_order(q, mask, negate, order)
    m = int(g('nvalid'))
    assert m == len(order), '%s: nvalid %d, oracle %d' % (what, m, len(order))
    perm = applied_permutation(g('acum'), m, payload_slab, n)
    if not np.array_equal(perm, order):
        bad = np.flatnonzero(perm != order)
        raise AssertionError('%s: permutation differs at %d of %d sorted positions, first at %d: cell %r, oracle %d'
                             % (what, len(bad), m, int(bad[0]), float(perm[bad[0]]), int(order[bad[0]])))
    assert np.array_equal(g('q_sorted')[:m], xs), what + ': q_sorted'
    return order, xs


def exact_Q(order, xs, targets, payload_slab=0, n=None):
    """Q of the integer payload: acum is exact on both sides, so the 'right' rule holds for EVERY target, no bracket"""
    if len(order) == 0:
        return np.full(len(targets), np.nan)
    acum = np.cumsum(order.astype(np.int64) + 1 + (payload_slab * n if payload_slab else 0)).astype(np.float64)
    assert acum[-1] < 2.0 ** 53
    idx = np.minimum(np.searchsorted(acum, np.asarray(targets, dtype=np.float64), side='right'), len(xs) - 1)
    return xs[idx]


def targets_for(order, J, rng):
    """J targets for the integer payload: half-integers, values that EQUAL an acum value (the only place the 'right' rule itself
    shows), targets below acum[0] and above acum[-1]"""
    acum = np.cumsum(order.astype(np.int64) + 1).astype(np.float64)
    m = len(acum)
    t = np.empty(J)
    pick = rng.integers(0, m, J)
    kind = np.arange(J) % 4
    t[:] = acum[pick]                                            # kind 0: exactly an acum value
    t[kind == 1] = acum[pick[kind == 1]] - 0.5                   # half-integers on either side of one
    t[kind == 2] = acum[pick[kind == 2]] + 0.5
    t[kind == 3] = np.floor(rng.random(int((kind == 3).sum())) * acum[-1]) + 0.5
    if J >= 8:
        t[3], t[4], t[5], t[6], t[7] = acum[0] - 0.5, -3.0, acum[-1] + 0.5, acum[-1] * 4, acum[0]
        t[1], t[2] = acum[-1], acum[m // 2]
    return t


def acum_longdouble(w, order):
    """cumulative sum of the sorted weights in long double (64-bit mantissa on x86): float64 np.cumsum itself drifts ~7e-14 of
    the total at 6.48 M cells, most of the 1e-12 the suite allows"""
    return np.cumsum(np.broadcast_to(w, w.shape).ravel()[order].astype(np.longdouble))


def rel_longdouble(acum, ref):
    """max |acum - ref| / ref over the cells, in long double"""
    a = np.asarray(acum, dtype=np.float64).astype(np.longdouble)
    return float(np.max(np.abs(a - ref) / np.abs(ref))) if len(ref) else 0.0


def bpe_longdouble(O, xs, ws, tbl, coord):
    """oracle.bpe_integral with the cumulative sum and the final sum in long double"""
    acum = np.cumsum(ws.astype(np.longdouble))
    tbl, coord = np.asarray(tbl, dtype=np.float64), np.asarray(coord, dtype=np.float64)
    z = O.interp1d((acum - 0.5 * ws).astype(np.float64), tbl, coord, O.table_increasing(tbl))
    return float(np.sum(xs.astype(np.longdouble) * z * ws))


# ---- K1 blocks and the groups of k_range_bounds (where a stray has to sit to fall to a given wave)
def minmax_blocks(ncell, nslab=1):
    """xc_internal.h minmax_blocks(): K1 blocks per slab"""
    p = min((ncell + 8191) // 8192, 1024)
    nslab = max(nslab, 1)
    if p * nslab < 2048:
        f = (ncell + 4095) // 4096
        if f * nslab > 2048:
            f = 2048 // nslab
        p = max(p, f)
    return max(1, min(p, 2048))


def range_groups(ncell, itemsize=8):
    """(ng, T, first cell of every group) of one plane.  K1 (xc_misc.hip k_minmax_partial) deals the plane's 16-byte vectors
    (2 float64 / 4 float32 cells; the staged plane is 16-byte aligned: no head) to its P blocks in contiguous shares of
    ceil(nvec / P) vectors; k_range_bounds folds `per = ceil(P / 512)` consecutive blocks into a group and hands group g to the
    thread with g == lane * 8 + wave -- group g is looked at by wave g % 8; T = 9 for 72 groups or more, else ng / 8, at least 1:
    strays in at most T - 1 groups per side are trimmed."""
    P = minmax_blocks(ncell)
    vn = 16 // itemsize
    nvec = ncell // vn
    perv = (nvec + P - 1) // P
    per = (P + 511) // 512
    ng = (P + per - 1) // per
    T = 9 if ng >= 72 else max(ng // 8, 1)
    first = np.minimum(np.arange(ng, dtype=np.int64) * per * perv, max(nvec - 1, 0)) * vn
    return ng, T, first


def stray_cells(ncell, count, one_wave):
    """one cell in each of `count` groups: all of them groups of wave 0 (g % 8 == 0), or dealt over the eight waves (g = 0, 1, ...)"""
    ng, T, first = range_groups(ncell)
    gs = np.arange(count) * 8 if one_wave else np.arange(count)
    assert gs[-1] < ng
    return first[gs] + 5


# ---- child process of test_sort_range_off_in_a_child_takes_path_0 (a fresh interpreter with XC_SORT_RANGE=0 in its environment)
def _child(out_path):
    sys.path.insert(0, ROOT)
    from xcontour_amd import _native
    ctx = _native.Context(0)
    res = {}
    for name, (q, mask) in child_cases().items():
        ny, nx = q.shape
        r = ctx.sort_profile(q, dA=int_payload(ny, nx), mask=mask, want_sorted=True, want_acum=True)
        m = int(r['nvalid'])
        res[name] = {'path': ctx.last_sort_path(), 'nvalid': m, 'perm': applied_permutation(r['acum'], m).astype(np.int64).tolist()}
    ctx.close()
    with open(out_path, 'w') as f:
        json.dump(res, f)


def child_cases():
    rng = np.random.default_rng(71)
    ny, nx = 193, 170
    q = np.round(rng.standard_normal((ny, nx)) + np.linspace(-2, 2, ny)[:, None], 2)         # smooth + noise, ties
    q[rng.random(q.shape) < 0.01] = np.nan
    mask = (rng.random((ny, nx)) > 0.3).astype(np.float64)
    q2 = rng.standard_normal((5, 1024))
    m2 = np.ones(q2.size); m2[rng.permutation(q2.size)[:q2.size - 1025]] = 0.0                # nvalid = 1025
    return {'field': (q, mask), 'nvalid_1025': (q2, m2.reshape(q2.shape))}


if __name__ == '__main__':
    _child(sys.argv[1])
