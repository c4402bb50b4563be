"""helpers shared by the -m gpu test files (no tests here)"""
import os

import numpy as np

import xcontour_oracle as O
from test_gpu_parity import rel, RTOL, TIGHT, LMIN_FLOOR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

NINE = ('ctr', 'area', 'intgrdS', 'latEq', 'dqdA', 'dintSdA', 'Leq2', 'Lmin', 'nkeff')

def check_nine(out, s, r, with_eq=False, tbl=None, tbl_coord=None, preY=None, nkeff_mask=1e5):
    """all nine result vectors of slab `s` against the oracle's dict `r`; given the table the kernel was given (and the
    `preY` it was given), also the epilogue stage by stage on the kernel's own sums (check_epilogue, contour dtype = r's)"""
    assert np.array_equal(out['counts'][s].astype(np.int64), r['counts'])
    assert np.array_equal(out['ctr'][s], r['ctr'].astype(np.float64))
    assert rel(out['area'][s], r['area']) < TIGHT and rel(out['intgrdS'][s], r['intgrdS']) < TIGHT
    for k in ('latEq', 'dqdA', 'dintSdA', 'Leq2'):
        assert rel(out[k][s], r[k]) < RTOL, k
    assert rel(out['Lmin'][s], r['Lmin'], LMIN_FLOOR) < RTOL
    ok = r['Lmin'] > LMIN_FLOOR
    assert rel(out['nkeff'][s][ok], r['nkeff'][ok]) < RTOL
    if with_eq:
        for k in ('ctr', 'area', 'intgrdS', 'latEq'):
            assert rel(out[k + '_eq'][s], r[k + '_eq']) < RTOL, k
    if tbl is not None:
        check_epilogue(out, s, tbl, tbl_coord, preY, r['ctr'].dtype.type, nkeff_mask)

def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)

def check_nine_det(out, s, r, tbl=None, tbl_coord=None, preY=None, nkeff_mask=1e5):
    """check_nine for the fixed-point sums.  Lmin = 2 pi R cos(latEq) of a contour that encloses all but ~1e-13 of the sphere
    is a 1e-4 m quantity on a 4e7 m scale whose value IS the rounding of the area sum (cos near 90 degrees): such contours
    (Lmin below one metre) are compared through latEq only."""
    assert np.array_equal(out['counts'][s].astype(np.int64), r['counts'])
    assert np.array_equal(out['ctr'][s], r['ctr'].astype(np.float64))
    assert rel(out['area'][s], r['area']) < TIGHT and rel(out['intgrdS'][s], r['intgrdS']) < TIGHT
    for k in ('latEq', 'dqdA', 'dintSdA', 'Leq2'):
        assert rel(out[k][s], r[k]) < RTOL, k
    ok = r['Lmin'] > 1.0
    assert rel(out['Lmin'][s][ok], r['Lmin'][ok]) < RTOL
    assert rel(out['nkeff'][s][ok], r['nkeff'][ok]) < RTOL
    if tbl is not None:
        check_epilogue(out, s, tbl, tbl_coord, preY, r['ctr'].dtype.type, nkeff_mask)

def same_bits(a, b, what=''):
    """a == b bit for bit: equal values, NaN at the same places, the same infinities, the same signs of zero (NaN payloads
    aside).  The message names the first element that differs."""
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    assert a.shape == b.shape, '%s: shapes %s != %s' % (what, a.shape, b.shape)
    ok = (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))
    if not ok.all():
        i = int(np.flatnonzero(~ok)[0])
        raise AssertionError('%s: %d of %d elements differ, first at [%d]: %r != %r (oracle)'
                             % (what, int((~ok).sum()), ok.size, i, float(a[i]), float(b[i])))


def ulp_distance(a, b):
    """Elementwise number of float64 steps between a and b (uint64).  +0 and -0 are the same number (0 steps); inf is one
    step past the largest finite value; NaN against NaN is 0 and NaN against anything else is the largest uint64."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    def ordered(x):                      # the doubles in their numeric order as int64 (-0 -> 0)
        i = bits(x)
        return np.where(i < 0, np.int64(-2 ** 63) - i, i)
    oa, ob = ordered(a), ordered(b)
    ua, ub = oa.view(np.uint64), ob.view(np.uint64)
    d = np.where(oa >= ob, ua - ub, ub - ua)             # modulo 2^64: exact, a difference of two int64 fits in uint64
    na, nb = np.isnan(a), np.isnan(b)
    return np.where(na | nb, np.where(na & nb, np.uint64(0), np.uint64(2 ** 64 - 1)), d.reshape(a.shape))


# Lmin = 2 pi R cos(latEq) is the one transcendental of the epilogue: device cos (ocml) against the host's.  The bar is on the cosine
# itself: the kernel's Lmin must be 2 pi R times the host's cos or one of its two float64 neighbours, rounded (check_lmin).  On Lmin
# that allows 0, 1 or 2 ulp (a 1-ulp change of cos moves the rounded product by 0 / 1 / 2 ulp: 19 / 71 / 10 % of 2e6 uniform
# latitudes).  Measured on an MI355X by the whole gpu suite (800 check_lmin calls, each by its largest distance): cos 0 ulp in 286,
# 1 ulp in 514; Lmin 0 ulp in 286, 1 ulp in 290, 2 ulp in 224 -- never more.
LMIN_ULP_SEEN, COS_ULP_SEEN = {}, {}


def check_lmin(lm, lat, what=''):
    """the kernel's Lmin of the kernel's latEq: 2 pi R cos(deg2rad(latEq)) with the device cos within 1 ulp of the host's"""
    lm, lat = np.asarray(lm, dtype=np.float64), np.asarray(lat, dtype=np.float64)
    sc = 2.0 * np.pi * O.Rearth                                              # latitude_lengths_at (utils.py:532)
    c = np.cos(np.deg2rad(lat))
    with np.errstate(all='ignore'):
        cand = [sc * c, sc * np.nextafter(c, -np.inf), sc * np.nextafter(c, np.inf)]
    same_bits(cand[0], O.latitude_lengths_at(lat), what + ' Lmin restated')
    hit = np.isnan(lm) & np.isnan(cand[0])
    for v in cand:
        hit |= bits(lm) == bits(v)
    d = ulp_distance(lm, cand[0])
    dmax = int(d.max()) if d.size else 0
    LMIN_ULP_SEEN[dmax] = LMIN_ULP_SEEN.get(dmax, 0) + 1
    cmax = 0 if ((bits(lm) == bits(cand[0])) | (np.isnan(lm) & np.isnan(cand[0]))).all() else 1
    COS_ULP_SEEN[cmax] = COS_ULP_SEEN.get(cmax, 0) + 1
    if not hit.all():
        i = int(np.flatnonzero(~hit)[0])
        raise AssertionError('%s Lmin: at [%d] %r is not 2 pi R cos(latEq) with cos within 1 ulp of the host\'s %r (%d ulp)'
                             % (what, i, float(lm[i]), float(cand[0][i]), int(d[i])))


def check_epilogue(out, s, tbl, tbl_coord, preY=None, ctr_dtype=np.float32, nkeff_mask=1e5, ctr=None, what=''):
    """The Keff epilogue (xc_finalize.h finalize_body) of slab `s` of a result dict, stage by stage,
    each stage recomputed with the oracle from the kernel's OWN output of the stage before -- so that summation order in
    the sums is never taken for an epilogue error, and an error shows at the stage where it is made:
      latEq                    <- area through the table the kernel was given        bit for bit
      dintSdA, dqdA            <- ctr (in the contour dtype), area, intgrdS           bit for bit
      Leq2                     <- the kernel's dintSdA, dqdA                          bit for bit
      Lmin                     <- the kernel's latEq                                  cos to 1 ulp (check_lmin)
      nkeff (+ the mask cut)   <- the kernel's Leq2, Lmin                             bit for bit
      the nine '_eq' vectors   <- the kernel's latEq and that vector                  bit for bit
    `out`: a plan / facade dict (names + '<name>_eq') or xc_keff_epilogue's (+ 'interp' (nslab, 9, npre)); `ctr`: the
    levels when `out` holds none."""
    g = lambda k: np.asarray(out[k][s], dtype=np.float64)
    ctr = g('ctr') if ctr is None else np.asarray(ctr, dtype=np.float64)
    c = ctr.astype(ctr_dtype)
    assert np.array_equal(c.astype(np.float64), ctr, equal_nan=True), what + ': levels not representable in the contour dtype'
    area, ints = g('area'), g('intgrdS')
    tbl, crd = np.asarray(tbl, dtype=np.float64), np.asarray(tbl_coord, dtype=np.float64)
    lat = g('latEq')
    with np.errstate(all='ignore'):
        same_bits(lat, O.lookup_coordinates(area, tbl, crd), what + ' latEq')
        same_bits(g('dintSdA'), O.cal_gradient_wrt_area(ints, area), what + ' dintSdA')
        same_bits(g('dqdA'), O.cal_gradient_wrt_area(c, area), what + ' dqdA')
        same_bits(g('Leq2'), O.cal_sqared_equivalent_length(g('dintSdA'), g('dqdA')), what + ' Leq2')
        lm = g('Lmin')
        check_lmin(lm, lat, what)
        same_bits(g('nkeff'), O.cal_normalized_Keff(g('Leq2'), lm, nkeff_mask), what + ' nkeff')
        if preY is None:
            return
        own = dict(ctr=c, area=area, intgrdS=ints, latEq=lat, dintSdA=g('dintSdA'), dqdA=g('dqdA'), Leq2=g('Leq2'), Lmin=lm,
                   nkeff=g('nkeff'))
        for i, k in enumerate(O.EQ_NAMES):
            eq = np.asarray(out['interp'][s, i] if 'interp' in out else out[k + '_eq'][s], dtype=np.float64)
            same_bits(eq, O.interp_to_coords(np.asarray(preY, dtype=np.float64), lat, own[k]), what + ' ' + k + '_eq')


def check_epilogue_equals(out, s, r, what=''):
    """The derived vectors of slab `s` against the oracle's `r`, computed from the SAME sums and the SAME table, at
    check_epilogue's bars: bit for bit, Lmin through check_lmin.  Where the two Lmin differ, nkeff (and Lmin_eq / nkeff_eq) differ
    with them: there check_epilogue (nkeff from the kernel's own Lmin) is what holds."""
    g = lambda k: np.asarray(out[k][s], dtype=np.float64)
    for k in ('latEq', 'dintSdA', 'dqdA', 'Leq2'):
        same_bits(g(k), r[k], what + ' ' + k)
    same_bits(g('latEq'), r['latEq'], what + ' latEq')
    check_lmin(g('Lmin'), r['latEq'], what)
    eq = ulp_distance(g('Lmin'), r['Lmin']) == 0
    same_bits(g('nkeff')[eq], r['nkeff'][eq], what + ' nkeff')
    for i, k in enumerate(O.EQ_NAMES):
        if k + '_eq' in r and (eq.all() or k not in ('Lmin', 'nkeff')):
            v = out['interp'][s, i] if 'interp' in out else out[k + '_eq'][s]
            same_bits(v, r[k + '_eq'], what + ' ' + k + '_eq')


def _clean_env():
    return {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT', 'XC_DIST_TOKEN')}
