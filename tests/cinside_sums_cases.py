"""The planes, term lists and placements behind test_gpu_cinside_sums.py, shared with the host tests (test_cinside_host.py,
test_cpinside_host.py) -- a helper, no tests here.  A test decides exactly which float64 terms K17 (xc_contour_interior_dev) or K18
(xc_contour_piece_interiors_dev) sums by writing them onto nodes it knows to be inside, on planes whose inside is plain:

  'k17 rows'       q[r][c] = r, periodic, select 2 (main), levels 1.5 (and 5.5): the inside is the rows above the level
  'k18 block'      a plain plane with one rectangular block ring (rows 2 .. ny - 2, columns 1 .. nx - 2), winding 0: the walks go DOWN
  'k18 comb down'  a periodic comb ring near the top of the plane, winding != 0, flip 0: the inside is below it, the walks go DOWN
  'k18 comb up'    a periodic comb ring near the bottom, winding != 0, flip 1: the inside is above it, the walks go UP

The records are traced by the restatements of K12 (contour_join_ref, contour_join_periodic_ref) from ONE slab and repeated per slab, so a
batch of cases is one call with one case per slab (w per slab, or f): every slab has its own windows.  Placements of a term list on the
inside nodes: 'lanes' consecutive columns of the first inside rows (the lanes of one wave of K17's scan, neighbouring walks of K18);
'strided' a stride of about 0.38 of the inside nodes, the first term in the last columns (on 70 columns: K17's partial second wave), so
consecutive terms lie in different waves, chunks of rows and walks; 'column' one column (one lane per chunk of K17, ONE walk of K18).
One OUTSIDE node holds the value that fixes the bound (`bound`), further outside nodes the values of `outside`; every other node holds
`background`.  No expected value comes from here but the ones written out (`want`): the tests take theirs from cinside_ref.interior and
cpinside_ref.piece_interiors."""
import functools
import math

import numpy as np

import cinside_ref as IR
import contour_join_periodic_ref as JP
import contour_join_ref as JR
import cpiece_records_ref as RR
import cpinside_ref as PR

SHAPES = ((12, 70), (70, 12))
KINDS = ('k17 rows', 'k18 block', 'k18 comb down', 'k18 comb up')
PLACEMENTS = ('lanes', 'strided', 'column')
TOP = 13                                 # the window of a slab whose bound is 1.5 (or 1.0, the weight of w = None)
p2 = RR.p2
ONE_UP = RR.ONE_UP


# ------------------------------------------------------------------ planes
@functools.lru_cache(maxsize=None)
def plane(kind, ny, nx, nlev=1):
    """-> dict(kind, ny, nx, periodic, select, flip, nlev, rec (the records of one slab, nlev ranges), masks bool (nlev, ny, nx), inner
    (the nodes inside EVERY range), outside (the nodes outside every range))"""
    assert kind in KINDS and nlev in (1, 2) and ny >= 8 and nx >= 8
    q = np.zeros((ny, nx))
    select = 0
    if kind == 'k17 rows':
        q[:] = np.arange(ny, dtype=np.float64)[:, None]
        levels, periodic, flip, select = (1.5, 5.5)[:nlev], 1, 0, 2
    elif kind == 'k18 block':
        q[2:ny - 1, 1:nx - 1] = 1.0
        levels, periodic, flip = (0.5, 0.75)[:nlev], 0, 0
    else:
        up = kind == 'k18 comb up'
        for c in range(nx):
            q[((ny - 4, ny - 2, ny - 3) if up else (2, 4, 3))[c % 3]:, c] = 1.0
        levels, periodic, flip = (0.5, 0.75)[:nlev], 1, int(up)
    rec = (JP if periodic else JR).stack_records(q[None], np.asarray(levels, dtype=np.float64))
    rec = (rec[0].ravel(),) + tuple(rec[1:])
    if kind == 'k17 rows':
        masks = IR.interior(*rec, ny, nx, periodic, select, flip=flip, ncont=nlev)['mask'].astype(bool)
        assert all(np.array_equal(m, q > lv) for m, lv in zip(masks, levels))
    else:
        tables, ms = PR.piece_interiors(*rec, ny, nx, periodic, flip=flip, ncont=nlev, return_masks=True)
        assert all(t.size == 1 and t['closed'][0] and (t['winding'][0] != 0) == bool(periodic) for t in tables)
        masks = np.array([m[0] for m in ms])
        assert all(np.array_equal(m, (q > 0.5) ^ bool(flip)) for m in masks)
    return dict(kind=kind, ny=ny, nx=nx, periodic=periodic, select=select, flip=flip, nlev=nlev, rec=rec, masks=masks,
                inner=masks.all(axis=0), outside=~masks.any(axis=0))


def records(pl, nslab):
    """the records of pl['rec'] once per slab (range = slab * nlev + level)"""
    cnt, ef, et, pts = pl['rec']
    return np.tile(cnt, nslab), np.tile(ef, nslab), np.tile(et, nslab), np.tile(pts, (nslab, 1))


def nodes_for(mask, n, how, start=0):
    """-> (rows, cols) of n inside nodes in the order the terms take them, or None where they do not fit"""
    assert how in PLACEMENTS
    if how == 'column':
        c = int(np.argmax(mask.sum(axis=0)))
        rows = np.flatnonzero(mask[:, c])
        return (rows[:n], np.full(n, c)) if n <= rows.size else None
    nodes = np.argwhere(mask)
    N = len(nodes)
    if n > N:
        return None
    if how == 'lanes':
        idx = (start + np.arange(n)) % N
    else:
        S = int(0.382 * N) | 1
        while math.gcd(S, N) != 1:
            S += 2
        idx = (N - 4 + (start + np.arange(n)) * S) % N
    return nodes[idx, 0], nodes[idx, 1]


def case(name, terms=None, bound=1.5, top=TOP, want=None, outside=(), background=0.0, every_inside=None, cut=False):
    """one slab: `terms` on inside nodes (or `every_inside` on all of them), `bound` on the first outside node, `outside` on the
    next ones, `background` elsewhere.  top: the window the slab must have; want: the sum written out (None: the reference's alone); cut:
    the case is about terms that straddle the bottom -- the expected sum must differ from plain fsum"""
    return dict(name=name, terms=None if terms is None else [float(t) for t in terms], bound=bound, top=top, want=want,
                outside=tuple(outside), background=background, every_inside=every_inside, cut=cut)


def fill(pl, cs, how, start=0):
    """the plane of one case -> float64 (ny, nx), or None where its terms do not fit"""
    v = np.full((pl['ny'], pl['nx']), float(cs['background']))
    if cs['every_inside'] is not None:
        v[pl['inner']] = cs['every_inside']
    if cs['terms'] is not None:
        at = nodes_for(pl['inner'], len(cs['terms']), how, start)
        if at is None:
            return None
        v[at] = cs['terms']
    out = np.argwhere(pl['outside'])
    assert len(out) > 3 * (1 + len(cs['outside']))
    for k, x in enumerate(([] if cs['bound'] is None else [cs['bound']]) + list(cs['outside'])):
        v[tuple(out[3 * k])] = x                                             # three nodes apart: different lanes of the bound's pass
    return v


def planes_for(kind, cases, how, nlev=1):
    """the smallest planes on which every case fits: both SHAPES where they do, else one tall plane (column) or 70 x 70"""
    n = max(len(c['terms'] or ()) for c in cases)
    fit = [plane(kind, ny, nx, nlev) for ny, nx in SHAPES]
    fit = [pl for pl in fit if nodes_for(pl['inner'], n, how) is not None]
    if not fit:
        fit = [plane(kind, n + 8, 12, nlev) if how == 'column' else plane(kind, 70, 70, nlev)]
        assert nodes_for(fit[0]['inner'], n, how) is not None
    return fit


def stack(pl, cases, how, vary=False):
    """-> float64 (ncase, ny, nx): slab k holds case k (vary: its terms start at inside node k of the placement's order)"""
    return np.array([fill(pl, c, how, k if vary else 0) for k, c in enumerate(cases)])


def float32_exact(v):
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(all='ignore'):
        return bool(np.all((v.astype(np.float32).astype(np.float64) == v) | np.isnan(v)))


# ------------------------------------------------------------------ the cases
def far_terms(n=40, seed=31):
    """signed terms with random 53-bit mantissas (first and last bit set) at 2^-40 and 2^-41"""
    rng = np.random.default_rng(seed)
    m = (rng.integers(0, 1 << 51, n, dtype=np.int64) << 1) | (1 << 52) | 1
    return (np.ldexp(m.astype(np.float64), rng.integers(-41, -39, n) - 52) * rng.choice([-1.0, 1.0], n)).tolist()


def ordinary_terms(n=40, seed=32):
    """signed full mantissas with exponents in [-20, 20]: the terms of the suites that stay in the middle of the window"""
    rng = np.random.default_rng(seed)
    return (np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(-20, 20, n)) * rng.choice([-1.0, 1.0], n)).tolist()


@functools.lru_cache(maxsize=None)
def batches():
    """name -> the cases of one call (one per slab).  Every slab's bound sits on an OUTSIDE node."""
    ex = RR.exact_cases()
    B = {}
    B['exact'] = [case(k, t, want=w) for k, (t, w) in ex.items() if k != 'absorption']
    B['absorption'] = [case('absorption', ex['absorption'][0], want=ex['absorption'][1])]
    B['shifts'] = [case('every shift', RR.every_shift_terms()), case('all ones', RR.all_ones_terms())]
    B['shifts alone'] = ([case('shift %d alone' % k, [t], want=t) for k, t in enumerate(RR.every_shift_terms())] +
                         [case('ones %d alone' % k, [t], want=t) for k, t in enumerate(RR.all_ones_terms())])
    b = TOP - RR.WINDOW_BITS
    straddling, whole = RR.bottom_terms(b)
    B['bottom'] = [case('bottom of the window', straddling, want=p2(b + 20) + p2(b), cut=True),
                   case('whole at the bottom', whole, want=whole[0]),
                   case('the leading bit alone survives', [math.ldexp(ONE_UP, b)], want=p2(b), cut=True),
                   case('just under the bottom', [math.ldexp(ONE_UP, b - 1), p2(b)], want=p2(b), cut=True),
                   case('53 bits under the bottom', [math.ldexp(ONE_UP, b - 53), -p2(b)], want=-p2(b), cut=True)]
    # the bound lies outside the region: 2^100 on an outside node, the terms near 2^-40 lose their bits under 2^(100 + 13 - 160)
    B['bound outside'] = [case('a far bound', far_terms(), bound=p2(100), top=113, cut=True)]
    big = 1.5 * p2(20)
    inf, nan = float('inf'), float('nan')
    B['non-finite'] = [case('non-finite values outside', ordinary_terms(), bound=big, top=33, outside=(inf, -inf, nan)),
                       case('an infinity inside', ordinary_terms() + [inf], bound=big, top=33, outside=(nan,)),
                       case('a negative infinity inside', ordinary_terms() + [-inf], bound=big, top=33, outside=(inf,)),
                       case('a NaN inside', ordinary_terms() + [nan], bound=big, top=33, outside=(-inf,))]
    B['high'] = [case(k + ' at 2^1000', [t * p2(1000) for t in ts], bound=1.5 * p2(1000), top=1013, want=w * p2(1000))
                 for k, (ts, w) in ex.items() if k != 'absorption']
    B['many equal'] = [case('ONE_UP on every inside node', bound=None, every_inside=ONE_UP),
                       case('-ONE_UP on every node', bound=None, every_inside=-ONE_UP, background=-ONE_UP)]
    return B


SPREAD_ONLY = ('shifts alone',)          # one term per slab: nothing to put into one column; term k starts at node k of the order
PLACED_ONCE = ('many equal',)            # every inside node holds the term: no placement


def runs(kind, batch):
    """the calls of one batch on one kind of plane -> [(what, pl, W float64 (ncase, ny, nx), cases)]"""
    cases = batches()[batch]
    out = []
    for how in PLACEMENTS:
        if (batch in SPREAD_ONLY and how != 'strided') or (batch in PLACED_ONCE and how != 'lanes'):
            continue
        fit = [plane(kind, 70, 12)] if batch in PLACED_ONCE else planes_for(kind, cases, how)
        for pl in fit:
            W = stack(pl, cases, how, vary=batch in SPREAD_ONLY)
            out.append(('%s, %s, %s, %d x %d' % (batch, kind, how, pl['ny'], pl['nx']), pl, W, cases))
    return out


def variants(W, cases):
    """the terms in w, again in a float64 f under w = None (weight 1), and in a float32 f for the slabs a float32 holds exactly
    -> [(name, w, f, the indices of the cases)]"""
    every = list(range(len(cases)))
    out = [('w', W, None, every), ('f64', None, W, every)]
    ok = [k for k in every if float32_exact(W[k])]
    if ok:
        out.append(('f32', None, W[ok].astype(np.float32), ok))
    return out


def inside_terms(pl, W, k, level=0):
    return W[k][pl['masks'][level]].tolist()


# ------------------------------------------------------------------ the cases with a w AND an f of their own
def floor_case(pl):
    """-> [(name, w (ny, nx), f (1, ny, nx) or None, what to expect)]: windows at the floor, top = -800, bottom = -960"""
    ny, nx = pl['ny'], pl['nx']
    rng = np.random.default_rng(33)
    ordinary = np.ldexp(rng.uniform(1.0, 2.0, (1, ny, nx)), rng.integers(-20, 20, (1, ny, nx)))
    zeros = np.zeros((ny, nx))
    zeros[::2, ::3] = -0.0
    den = np.ldexp(rng.integers(1, 1 << 50, (ny, nx)).astype(np.float64), -1074) * rng.choice([-1.0, 1.0], (ny, nx))
    assert (np.abs(den) < 2.0 ** -1022).all() and (den != 0.0).all()
    out = [('all weights zero', zeros, ordinary, dict(sum_w=0.0, sum_wf=0.0)),
           ('all weights denormal', den, np.ones((1, ny, nx)), dict(sum_w=0.0, sum_wf=0.0)),
           ('all weights NaN', np.full((ny, nx), np.nan), ordinary, dict(sum_w=0.0, sum_wf=0.0))]
    # the largest weight 2^-900: terms there survive whole, a term at 2^-1000 is dropped, a denormal product is dropped; what survives
    # cancels down to 2^-952, so that either dropped term would show in the sum
    terms = [math.ldexp(ONE_UP, -900), -p2(-900), math.ldexp(ONE_UP, -1000), -p2(-900), p2(-900)]
    cs = case('the largest weight is 2^-900', terms, bound=1.5 * p2(-900), top=-800)
    w = fill(pl, cs, 'strided')
    f = np.ones((1, ny, nx))
    at = nodes_for(pl['inner'], len(terms), 'strided')
    f[0, at[0][1], at[1][1]] = 3.0                                           # -3 2^-900
    f[0, at[0][3], at[1][3]] = p2(-150)                                      # -2^-1050, a denormal product: dropped
    f[0, at[0][4], at[1][4]] = 2.0                                           # 2^-899
    out.append((cs['name'], w, f, dict(sum_w=p2(-952), sum_wf=p2(-952))))
    return out


def per_slab_case(pl, what):
    """two slabs, each with the sticky-tie case inside, 2^120 apart -> (w, f, tops [(top_w, top_f)] per slab, want per slab):
    'f': one shared 2-D w of ones, f[0] at 2^-60, f[1] at 2^+60;  'w': a 3-D w whose slabs are 2^-60 and 2^+60, no f"""
    terms, want = RR.exact_cases()['sticky lifts the tie']
    V = np.array([fill(pl, case('s', [t * p2(e) for t in terms], bound=1.5 * p2(e)), 'strided') for e in (-60, 60)])
    if what == 'f':
        return np.ones((pl['ny'], pl['nx'])), V, [(13, -47), (13, 73)], [want * p2(-60), want * p2(60)]
    return V, None, [(-47, None), (73, None)], [want * p2(-60), want * p2(60)]


def float32_integrand_case(pl, seed=34):
    """w with full mantissas on every node and a float32 f -> (w, f); the products must be taken in float64 after the cast"""
    rng = np.random.default_rng(seed)
    ny, nx = pl['ny'], pl['nx']
    w = np.ldexp(rng.uniform(1.0, 2.0, (ny, nx)), rng.integers(-3, 3, (ny, nx)))
    f = (np.ldexp(rng.uniform(1.0, 2.0, (1, ny, nx)), rng.integers(-3, 3, (1, ny, nx))) * rng.choice([-1.0, 1.0], (1, ny, nx))).astype(np.float32)
    return w, f


def overflow_case(pl, inside):
    """ordinary w and f but for one node with w = 2^1000 and f = 2^100, whose product overflows -> (w, f)"""
    ny, nx = pl['ny'], pl['nx']
    rng = np.random.default_rng(35)
    w = np.ldexp(rng.uniform(1.0, 2.0, (ny, nx)), rng.integers(-20, 20, (ny, nx)))
    f = np.ldexp(rng.uniform(1.0, 2.0, (1, ny, nx)), rng.integers(-20, 20, (1, ny, nx))) * rng.choice([-1.0, 1.0], (1, ny, nx))
    r, c = np.argwhere(pl['inner'] if inside else pl['outside'])[5]
    w[r, c], f[0, r, c] = p2(1000), p2(100)
    return w, f


# ------------------------------------------------------------------ broken bound rules, for the host tests
def bound_with_infinities(v):
    """the largest |v| over the entries that are not NaN, an infinity counting as the largest float64"""
    a = np.abs(np.asarray(v, dtype=np.float64).ravel())
    a = a[~np.isnan(a)]
    return float(min(a.max(), np.finfo(np.float64).max)) if a.size else 0.0


def bound_over(mask):
    """the largest finite |v| over the nodes of `mask` alone"""
    return lambda v: IR.finite_bound(np.asarray(v)[mask])


def reference(pl, nslab, w=None, f=None, tops=None):
    """the reference of one call on pl's records -> (per range sum_w, sum_wf (None without f), n_in; per slab the tops)"""
    rec = records(pl, nslab)
    if pl['kind'] == 'k17 rows':
        r = IR.interior(*rec, pl['ny'], pl['nx'], pl['periodic'], pl['select'], flip=pl['flip'], ncont=pl['nlev'], w=w, f=f, tops=tops)
        return r['sum_w'], r['sum_wf'], r['n_in'], r['tops']
    t, tp = PR.piece_interiors(*rec, pl['ny'], pl['nx'], pl['periodic'], flip=pl['flip'], ncont=pl['nlev'], w=w, f=f, return_tops=True, tops=tops)
    assert all(x.size == 1 for x in t)
    return (np.array([x['sum_w'][0] for x in t]), None if f is None else np.array([x['sum_wf'][0] for x in t]),
            np.array([x['n_in'][0] for x in t]), tp)


# ------------------------------------------------------------------ the limb model on the derived windows, for the host tests
def same(a, b):
    return IR.same_bits(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))


def limb_model_report(kind):
    """Every term list of every batch on `kind`'s planes, every placement: the reference's sum_w (terms in w) and sum_wf (terms in f
    under weight 1) against the sound limb model on the windows of window_tops, against the written-out `want`, and -- for a case
    about the cut -- against plain fsum, from which it must differ.  -> (defect -> the names of the cases that fail under it, the
    number of term lists seen)"""
    caught, seen = {d: set() for d in RR.DEFECTS}, 0
    for batch in batches():
        for what, pl, W, cases in runs(kind, batch):
            for vname, w, f, which in variants(W, cases):
                if vname == 'f32':
                    continue                                                 # the same float64 terms as f64
                sw, swf, n_in, tops = reference(pl, len(cases), w=w, f=f)
                got = sw if vname == 'w' else swf
                assert n_in.tolist() == [int(pl['masks'][0].sum())] * len(cases), what
                for k, cs in enumerate(cases):
                    where = (what, vname, cs['name'])
                    top = tops[k][0 if vname == 'w' else 1]
                    assert top == cs['top'] and tops[k][0] == (cs['top'] if vname == 'w' else TOP), where
                    terms = [t for t in inside_terms(pl, W, k) if not math.isnan(t)]
                    if cs['terms'] is not None:
                        assert sorted(t for t in terms if t != 0.0) == sorted(t for t in cs['terms'] if t == t and t != 0.0), where
                    seen += 1
                    if any(math.isinf(t) for t in terms):
                        assert math.isnan(got[k]), where
                        continue
                    assert same(got[k], RR.limb_sum(terms, top)) and same(got[k], RR.limb_sum(terms[::-1], top)), where
                    if cs['want'] is not None:
                        assert same(got[k], cs['want']), where
                    assert (not same(got[k], math.fsum(terms))) == cs['cut'], where
                    for d in RR.DEFECTS:
                        if not same(RR.limb_sum(terms, top, d), got[k]):
                            caught[d].add(cs['name'])
    return caught, seen


CATCHES = {                              # the term lists written for a defect of the accumulator do catch it, on K17's and K18's windows
    'ties away from zero': {'tie to even, down', 'negative tie to even', 'tie to even, down at 2^1000'},
    'ties toward zero': {'tie to even, up', 'borrow, tie to even', 'tie to even, up at 2^1000'},
    'no sticky bit': {'sticky lifts the tie', 'negative sticky', 'sticky lifts the tie at 2^1000'},
    'a carry lost between limbs': {'absorption', 'borrow through three limbs', 'borrow, exact', 'ONE_UP on every inside node'},
    'no borrow on a negative sum': {'all limbs negative', 'negative borrow', '-ONE_UP on every node', '53 bits under the bottom'},
    'a chunk one limb off at shift 17': {'ones 13 alone', 'ones 45 alone', 'ones 77 alone'},
}
