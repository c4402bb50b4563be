"""The planes, placements and calls behind test_gpu_ring_sums.py, shared with test_ring_sums_host.py -- a helper, no tests here.  The
sums of K19 (xc_contour_piece_tree_dev: gross and net), K21 (xc_contour_piece_props_dev: net and gross of every field) and K22
(xc_label_overlap_dev: sum_w, sum_wf) at the edges of their windows.  The term lists are cinside_sums_cases' (batches(), floor_case, the
float32 and the overflow case): a test decides which float64 terms land in which sum by writing them onto the TARGET nodes of a plane.

  K22  maps()   rows 0 and 1 are the omitted pair (-1, -1), rows 2 .. ny - 4 the target pair (2, 5), row ny - 3 the one-sided pair
                (2, -9) -> (2, -1), the last two rows the pair (7, 5).  The node that fixes the bound lies in the omitted rows
                ('omitted') or in the pair (7, 5) ('other pair'): the bound is taken over the whole plane either way.
  K19 / K21     rings(): 'chain' cptree_cases.chain(17), eight nested square rings, the target the second largest (48 net nodes: it has
                a parent and six descendants); 'nest' a block, a hole one node inside it and a 2 x 2 island in the hole's middle, the
                target the hole (the planes for the lists that need more nodes); 'round' a periodic plane whose rows >= 2 lie inside a
                ring that goes round, with a hole and an island below row 17, the target the ring that goes round.  The records come
                from the K12 restatements, once per slab, as cinside_sums_cases.plane's.  The bound's node lies outside every ring.

Placements (PLACEMENTS): 'column' one column of the target (one thread's private words and its runs); 'lanes' consecutive columns of
the target's first rows; 'strided' a stride of about 0.38 of the target's nodes, the first term near the end; 'full wave' the 'lanes'
order on planes of 64 and 128 columns whose waves lie whole in the target -- maps(33, 128) and rings('round', 33, 64 | 128) -- the one
placement in which the waves add their lanes' words with shuffles.  One case per slab: one call checks a batch.

model(): the chain the three kernels share, in Python integers -- a term cut into 32-bit chunks at the window's floor (cp_split), the
private words of a thread's run, the wave's sum at the chunk's end, the staged words, K19's subtraction of the children and K21's fold
up the tree, the carry and the one rounding (cp_to_double) -- with DEFECTS that each break one step.  model_report() runs it over every
call of a kernel: the sound model equals the restatement bit for bit, and every defect is caught by some call."""
import functools
import math
from fractions import Fraction

import numpy as np

import cinside_ref as IR
import cinside_sums_cases as SC
import contour_join_periodic_ref as JP
import contour_join_ref as JR
import cpiece_records_ref as RR
import cplabel_ref as LR
import cpoverlap_ref as OR
import cpprops_ref as QR
import cptree_cases as CS
import cptree_ref as TR

KERNELS = ('k19', 'k21', 'k22')
PLACEMENTS = ('column', 'lanes', 'strided', 'full wave')
ORDER = {'column': 'column', 'lanes': 'lanes', 'strided': 'strided', 'full wave': 'lanes'}   # cinside_sums_cases.nodes_for's orders
PAIR, ONE_SIDED, OTHER = (2, 5), (2, -1), (7, 5)
p2, ONE_UP = SC.p2, SC.ONE_UP
ALL_ONES = 2.0 - p2(-52)                 # all 53 mantissa bits set


# ------------------------------------------------------------------ planes
@functools.lru_cache(maxsize=None)
def maps(ny, nx, bound_in='omitted', nlev=1):
    assert ny >= 8 and bound_in in ('omitted', 'other pair', 'one pair')
    la, lb = np.full((ny, nx), -1, dtype=np.int32), np.full((ny, nx), -1, dtype=np.int32)
    if bound_in == 'one pair':                                               # the whole plane is the target pair
        la[:], lb[:] = PAIR
        outside = np.zeros((ny, nx), dtype=bool)
    else:
        la[2:ny - 3], lb[2:ny - 3] = PAIR
        la[ny - 3], lb[ny - 3] = 2, -9
        la[ny - 2:], lb[ny - 2:] = OTHER
        outside = (la == -1) & (lb == -1) if bound_in == 'omitted' else (la == OTHER[0])
    inner = (la == PAIR[0]) & (lb == PAIR[1])
    return dict(kind='k22', name='maps, bound in %s' % bound_in, ny=ny, nx=nx, periodic=0, flip=0, nlev=nlev, la=la, lb=lb, inner=inner,
                masks=inner[None], outside=outside, kept=~((la == -1) & (lb == -1)))


@functools.lru_cache(maxsize=None)
def rings(kind, ny, nx, nlev=1):
    """-> dict(.., rec the records of one slab (nlev ranges), table / ring_masks cptree_ref's of one range, labels cplabel_ref's, target
    the target's row in the table, inner its net nodes, outside the nodes outside every ring)"""
    q = np.zeros((ny, nx))
    periodic = 0
    if kind == 'chain':
        assert ny == nx
        q, size = CS.chain(ny), (ny - 4) ** 2
    elif kind == 'nest':
        assert ny >= 8 and nx >= 8
        q[1:ny - 1, 1:nx - 1] = 1.0
        q[2:ny - 2, 2:nx - 2] = 0.0
        q[ny // 2 - 1:ny // 2 + 1, nx // 2 - 1:nx // 2 + 1] = 1.0
        size = (ny - 4) * (nx - 4)
    else:
        assert kind == 'round' and ny >= 30 and nx >= 12
        periodic = 1
        q[2:] = 1.0
        q[18:ny - 3, nx // 2 - 4:nx // 2 + 4] = 0.0
        q[21:23, nx // 2 - 1:nx // 2 + 1] = 1.0
        size = (ny - 2) * nx
    rec = (JP if periodic else JR).stack_records(q[None], np.asarray((0.5, 0.75)[:nlev], dtype=np.float64))
    rec = (rec[0].ravel(),) + tuple(rec[1:])
    tabs, ms = TR.piece_tree(*rec, ny, nx, periodic, return_masks=True)
    assert all(t.tobytes() == tabs[0].tobytes() for t in tabs) and tabs[0]['closed'].all() and tabs[0].size >= 3
    t, ms = tabs[0], ms[0]
    (target,) = np.flatnonzero(t['n_in'] == size)
    labels = LR.labels_of_masks(ms, (ny, nx))
    assert (t['winding'][target] != 0) == (kind == 'round') and t['nchild'][target] == 1
    return dict(kind=kind, name='%s %d x %d' % (kind, ny, nx), ny=ny, nx=nx, periodic=periodic, flip=0, nlev=nlev, rec=rec, table=t,
                ring_masks=ms, labels=labels, target=int(target), inner=labels == target, masks=(labels == target)[None],
                outside=~np.any(ms, axis=0))


def records(pl, nslab):
    return SC.records(pl, nslab)


def fits(pl, n, how):
    return SC.nodes_for(pl['inner'], n, ORDER[how]) is not None


def planes_for(kernel, n, how):
    """the smallest planes whose target holds n terms in the placement"""
    if kernel == 'k22':
        if how == 'full wave':
            c = [lambda: maps(33, 128), lambda: maps(70, 128, 'other pair')]
        elif how == 'column':
            c = [lambda: maps(70, 12, 'other pair'), lambda: maps(n + 8, 12)]
        elif how == 'lanes':
            c = [lambda: maps(12, 70), lambda: maps(70, 70)]
        else:
            c = [lambda: maps(70, 12, 'other pair'), lambda: maps(70, 70, 'other pair')]
        first = 1
    else:
        if how == 'full wave':
            c = [lambda: rings('round', 33, 64), lambda: rings('round', 33, 128), lambda: rings('round', 70, 128)]
            first = 1 if kernel == 'k19' else 2                              # (K19's sums come from K18's walks: no wave adds anything)
        elif how == 'column':
            c, first = [lambda: rings('chain', 17, 17), lambda: rings('nest', n + 8, 12)], 1
        else:
            c, first = [lambda: rings('chain', 17, 17), lambda: rings('nest', 12, 70), lambda: rings('nest', 70, 70)], 1
    out = [pl for pl in (mk() for mk in c[:first]) if fits(pl, n, how)]
    for mk in c[first:]:
        if out:
            break
        out = [pl for pl in [mk()] if fits(pl, n, how)]
    assert out, (kernel, n, how)
    return out


def stack(pl, cases, how, vary=False):
    return np.array([SC.fill(pl, c, ORDER[how], k if vary else 0) for k, c in enumerate(cases)])


# ------------------------------------------------------------------ one call: the inputs, the windows, the restatement
def call(kernel, pl, nslab, w=None, f=None, fields=None, what='', lists=None):
    """the description of one call: w None, (ny, nx) or (nslab, ny, nx); f (nslab, ny, nx) or None (K19, K22); fields a list (K21)"""
    assert kernel in KERNELS and (fields is None) == (kernel != 'k21')
    return dict(kernel=kernel, pl=pl, nslab=nslab, w=w, f=f, fields=fields, what=what, lists=lists)


def fields_of(pl, nslab, w, f):
    """K21's five fields for a list that K19 and K22 take as (w, f): with the list in w five planes of ones, shared and per slab, float64
    and float32; else the list's plane as fields 0, 2 and 4 (field 4 runs in the scan's second pass) between planes of ones"""
    ny, nx = pl['ny'], pl['nx']
    ones = [np.ones((ny, nx)), np.ones((nslab, ny, nx), dtype=np.float32)]
    return [ones[0], ones[1], ones[0], ones[1], np.ones((nslab, ny, nx))] if f is None else [f, ones[0], f, ones[1], f]


def tops_of(c, bound=IR.finite_bound):
    """the windows of a call by the bound rule (cinside_ref.window_tops): per slab (top_w, top_f), for K21 per slab the tops of the fields"""
    pl = c['pl']
    if c['kernel'] == 'k21':
        return QR.field_tops(c['w'], c['fields'], c['nslab'], pl['ny'], pl['nx'], bound)
    return IR.window_tops(c['w'], c['f'], c['nslab'], pl['ny'], pl['nx'], bound)


def slab_of(a, s):
    return None if a is None else (a[s] if np.ndim(a) == 3 else a)


def restatement(c, tops=None):
    """-> per range a dict of float64 arrays: K19 sum_w, sum_wf, net_w, net_wf over the table's rows; K21 net, gross (rows, nf); K22 the
    rows' a, b, n, sum_w, sum_wf"""
    pl, ns, nlev = c['pl'], c['nslab'], c['pl']['nlev']
    tops = tops_of(c) if tops is None else tops
    if c['kernel'] == 'k22':
        out = []
        for r in range(ns * nlev):
            t = OR.overlap_of_maps(pl['la'], pl['lb'], slab_of(c['w'], r // nlev), slab_of(c['f'], r // nlev), tops=tops[r // nlev])
            out.append({k: t[k] for k in OR.DTYPE.names})
        return out
    rec = records(pl, ns)
    if c['kernel'] == 'k19':
        tabs = TR.piece_tree(*rec, pl['ny'], pl['nx'], pl['periodic'], ncont=nlev, w=c['w'], f=c['f'], tops=tops)
        return [{k: t[k] for k in TR.SUM_FIELDS} for t in tabs]
    _, props = QR.piece_props(*rec, pl['ny'], pl['nx'], pl['periodic'], ncont=nlev, w=c['w'], fields=c['fields'], tops=tops)
    return [dict(net=p['net'], gross=p['gross']) for p in props]


def same(a, b):
    return SC.same(a, b)


def target_of(c, res, r, column):
    """the target's value in one range's dict of restatement() (or of the GPU's results in the same form).  column: 'w' or 'f' -- K19
    (gross, net); K21 (gross, net) of field 0; K22 the pair's sum"""
    pl = c['pl']
    if c['kernel'] == 'k22':
        (row,) = np.flatnonzero((res[r]['a'] == PAIR[0]) & (res[r]['b'] == PAIR[1]))
        return (float(res[r]['sum_w' if column == 'w' else 'sum_wf'][row]),)
    if c['kernel'] == 'k19':
        return float(res[r]['sum_' + ('w' if column == 'w' else 'wf')][pl['target']]), float(res[r]['net_' + ('w' if column == 'w' else 'wf')][pl['target']])
    return float(res[r]['gross'][pl['target'], 0]), float(res[r]['net'][pl['target'], 0])


# ------------------------------------------------------------------ the calls of the term lists
def batch_calls(kernel, batch, hows=PLACEMENTS):
    """-> [(how, call, cases, vname, which)]: every list of the batch, one per slab, in w, in a float64 f and in a float32 f"""
    cases = SC.batches()[batch]
    n = max(len(c['terms'] or ()) for c in cases)
    out = []
    for how in hows:
        if (batch in SC.SPREAD_ONLY and how != 'strided') or (batch in SC.PLACED_ONCE and how not in ('lanes', 'full wave')):
            continue
        if batch in SC.PLACED_ONCE:
            fit = ([maps(33, 128)] if kernel == 'k22' else [rings('round', 33, 64)]) if how == 'full wave' else \
                  ([maps(70, 12, 'other pair')] if kernel == 'k22' else [rings('nest', 70, 12)])
        else:
            fit = planes_for(kernel, n, how)
        for pl in fit:
            W = stack(pl, cases, how, vary=batch in SC.SPREAD_ONLY)
            for vname, w, f, which in SC.variants(W, cases):
                what = '%s, %s, %s, %s, %s' % (batch, kernel, how, pl['name'], vname)
                fields = fields_of(pl, len(which), w, f) if kernel == 'k21' else None
                c = call(kernel, pl, len(which), w=(w if kernel != 'k21' or f is None else None), f=None if kernel == 'k21' else f,
                         fields=fields, what=what, lists=W[which])
                out.append((how, c, cases, vname, which))
    return out


def list_terms(c, j):
    """the float64 terms the target of slab j holds"""
    return c['lists'][j][c['pl']['inner']].tolist()


# ------------------------------------------------------------------ the calls with a w AND an f of their own
def as_call(kernel, pl, nslab, w, f, what):
    """(w, f) as K19 and K22 take them; K21 takes a field of ones (its sum is sum_w) and f as fields 0 and 1"""
    if kernel != 'k21':
        return call(kernel, pl, nslab, w=w, f=f, what=what)
    ny, nx = pl['ny'], pl['nx']
    return call(kernel, pl, nslab, w=w, fields=[np.ones((ny, nx))] + ([] if f is None else [f]), what=what)


def floor_planes(kernel):
    if kernel == 'k22':
        return [maps(12, 70), maps(12, 70, 'other pair'), maps(70, 12), maps(70, 12, 'other pair'), maps(33, 128), maps(33, 128, 'other pair')]
    return [rings('chain', 17, 17), rings('nest', 12, 70), rings('round', 33, 64)]


def floor_calls(kernel):
    """-> [(call, want dict(sum_w, sum_wf))]: cinside_sums_cases.floor_case on every plane of the kernel"""
    return [(as_call(kernel, pl, 1, w, f, 'floor: %s, %s, %s' % (name, kernel, pl['name'])), want)
            for pl in floor_planes(kernel) for name, w, f, want in SC.floor_case(pl)]


def per_slab_planes(kernel):
    if kernel == 'k22':
        return [maps(12, 70, 'omitted', 2), maps(70, 12, 'other pair', 2)]
    return [rings('chain', 17, 17, 2), rings('round', 33, 64, 2)]


def per_slab_calls(kernel):
    """two slabs whose bounds differ by 2^60 (1.5 2^-30 and 1.5 2^30), two ranges per slab, the sticky-tie list in each: a shared plane
    of ones as w with a per-slab f, and a per-slab w without f -> [(call, column, tops per slab, want per slab)]"""
    terms, want = RR.exact_cases()['sticky lifts the tie']
    out = []
    for pl in per_slab_planes(kernel):
        V = np.array([SC.fill(pl, SC.case('s', [t * p2(e) for t in terms], bound=1.5 * p2(e)), 'strided') for e in (-30, 30)])
        wants = [want * p2(-30), want * p2(30)]
        out.append((as_call(kernel, pl, 2, np.ones((pl['ny'], pl['nx'])), V, 'per-slab windows in f, %s, %s' % (kernel, pl['name'])), 'f',
                    [(13, -17), (13, 43)], wants))
        out.append((as_call(kernel, pl, 2, V, None, 'per-slab windows in w, %s, %s' % (kernel, pl['name'])), 'w', [(-17, None), (43, None)], wants))
    return out


FIELD_SPREAD = (40, -40, 20, -20)        # the exponents of the bounds of fields 0, 3, 4 and 7, rotated slab by slab
SMALL = p2(-110)                         # under the floor 2^(40 + 13 - 160) of the field whose bound is 1.5 2^40, inside every other window


def per_field_call(pl, nf):
    """K21: slab j gives field k_j = (0, 3, 4, 7)[j] (the ones below nf) the bound 1.5 2^40 and the others of these 1.5 2^-40, 1.5 2^20,
    1.5 2^-20; every other field 1.5.  Every field holds 2^e, -2^e and SMALL on the target: SMALL is lost in field k_j alone.
    -> (call, the k_j, tops per slab, want (nslab, nf))"""
    marked = [m for m in (0, 3, 4, 7) if m < nf]
    ns, ny, nx = len(marked), pl['ny'], pl['nx']
    fields = [np.empty((ns, ny, nx)) for _ in range(nf)]
    tops, want = [[13] * nf for _ in range(ns)], np.full((ns, nf), SMALL)
    for j, k in enumerate(marked):
        expo = {m: FIELD_SPREAD[(marked.index(m) - j) % len(marked)] for m in marked}
        assert expo[k] == 40
        for m in range(nf):
            e = expo.get(m, 0)
            fields[m][j] = SC.fill(pl, SC.case('field', [p2(e), -p2(e), SMALL], bound=1.5 * p2(e)), 'strided', start=m)
            tops[j][m] = e + 13
        want[j, k] = 0.0
    return call('k21', pl, ns, fields=fields, what='per-field windows, nf %d, %s' % (nf, pl['name'])), marked, tops, want


def float32_call(kernel, pl):
    w, f = SC.float32_integrand_case(pl)
    return as_call(kernel, pl, 1, w, f, 'float32 integrand, %s, %s' % (kernel, pl['name']))


def overflow_call(kernel, pl, inside):
    w, f = SC.overflow_case(pl, inside)
    return as_call(kernel, pl, 1, w, f, 'w f overflows %s, %s, %s' % ('inside' if inside else 'outside', kernel, pl['name']))


def no_wrap_planes(kernel):
    return [maps(70, 128, 'one pair')] if kernel == 'k22' else [rings('nest', 70, 128), rings('round', 70, 128)]


def no_wrap_calls(kernel):
    """every target node holds ALL_ONES, the largest term its window admits (it is the bound: top 13), slab 0 with +, slab 1 with -; once
    in w and once in a float64 f -> [(call, column, the number of target nodes)]"""
    out = []
    for pl in no_wrap_planes(kernel):
        V = np.array([np.where(pl['inner'], s * ALL_ONES, 0.0) for s in (1.0, -1.0)])
        n = int(pl['inner'].sum())
        out.append((as_call(kernel, pl, 2, V, None, 'no wrap in w, %s, %s' % (kernel, pl['name'])), 'w', n))
        out.append((as_call(kernel, pl, 2, None, V, 'no wrap in f, %s, %s' % (kernel, pl['name'])), 'f', n))
    return out


FOLD_B, FOLD_T, FOLD_G = ALL_ONES * p2(40), ALL_ONES * p2(-60), ONE_UP * p2(-30)


def fold_call(kernel):
    """the chain of rings: the target's child holds +B on a net node, the target -B and t on two of its own, the target's parent G; every
    other node 0.  B = ALL_ONES 2^40 is the bound: top 53, floor 2^-107, so t = ALL_ONES 2^-60 is cut there (its last five bits).
    -> (call, dict(child, target, parent: rows of the table), dict(t_cut, parent_gross))"""
    pl = rings('chain', 17, 17)
    t, lab = pl['table'], pl['labels']
    target = pl['target']
    (child,) = np.flatnonzero(t['parent'] == target)
    parent = int(t['parent'][target])
    v = np.zeros((1, 17, 17))
    at = {k: np.argwhere(lab == k) for k in (child, target, parent)}
    v[0][tuple(at[child][3])] = FOLD_B
    v[0][tuple(at[target][5])], v[0][tuple(at[target][20])] = -FOLD_B, FOLD_T
    v[0][tuple(at[parent][7])] = FOLD_G
    t_cut = RR.cut(FOLD_T, 53 - RR.WINDOW_BITS)
    assert t_cut != FOLD_T and t_cut != 0.0
    c = as_call(kernel, pl, 1, v[0], None, 'fold in w, %s' % kernel) if kernel == 'k19' else call('k21', pl, 1, fields=[v, np.ones((17, 17))], what='fold, k21')
    return c, dict(child=int(child), target=target, parent=parent), dict(t_cut=t_cut, parent_gross=math.fsum([t_cut, FOLD_G]))


# ------------------------------------------------------------------ the model of the chain, sound and broken
DEFECTS = ('rounds at the floor', 'keeps a term under the window', 'one window for all slabs', 'one window for all fields',
           'the tops of fields 4 to 7 from fields 0 to 3', 'the float32 integrand multiplied in float32', 'the wave sum in 32 bits',
           'a carry lost between two words', 'gross folded from rounded doubles', 'the bound over the kept nodes only',
           'a chunk one limb off at shift 17')
ONLY = {'one window for all fields': ('k21',), 'the tops of fields 4 to 7 from fields 0 to 3': ('k21',),
        'gross folded from rounded doubles': ('k21',), 'the bound over the kept nodes only': ('k22',), 'the wave sum in 32 bits': ('k21', 'k22')}
W64 = 1 << 64


@functools.lru_cache(maxsize=1 << 16)
def split(v, top, defect=None):
    """cp_split and the limbs its chunks go to: -> (False for a term that is not finite or lies above the window, ((limb, signed chunk), ..))"""
    if math.isinf(v):
        return False, ()
    if v == 0.0 or abs(v) < p2(-1022):
        return True, ()
    m, e = math.frexp(abs(v))
    M, sh = int(math.ldexp(m, 53)), (e - 53) - (top - RR.WINDOW_BITS)
    if sh < 0:
        if -sh >= 53 and defect != 'keeps a term under the window':
            return True, ()
        n = -sh & 63 if -sh >= 53 else -sh                                   # (the hardware's shift count without the early return)
        M = (M + (1 << (n - 1))) >> n if defect == 'rounds at the floor' and n else M >> n
        sh = 0
    k, s = divmod(sh, 32)
    big, ok, out = M << s, True, []
    for t, c in enumerate((big & 0xffffffff, (big >> 32) & 0xffffffff, big >> 64)):
        j = 4 - k - t
        if defect == 'a chunk one limb off at shift 17' and s == 17 and t == 1:
            j += 1
        if j < 0 or j > 4:
            ok = ok and c == 0
        elif c:
            out.append((j, -c if v < 0 else c))
    return ok, tuple(out)


def add_private(acc, v, top, defect=None):
    """cp_add_private: the chunks of one term into five words (mod 2^64); False where cp_add would flag"""
    ok, chunks = split(float(v), top, defect)
    for j, c in chunks:
        acc[j] = (acc[j] + c) % W64
    return ok


def to_double(acc, top, defect=None):
    """cp_to_double: the words carried, the exact value rounded once, half to even"""
    w = [a - W64 if a >= W64 // 2 else a for a in acc]
    for j in range(4, 0, -1):
        c = w[j] >> 32
        w[j] -= c << 32
        if not (defect == 'a carry lost between two words' and j == 2):
            w[j - 1] += c
    total = sum(w[j] << (32 * (4 - j)) for j in range(5))
    return RR.round_exact(Fraction(total) * Fraction(2) ** (top - RR.WINDOW_BITS))


def run_words(member, terms, top, rows, defect=None, waves=True):
    """the staged words of one set of nodes: a thread per (chunk of `rows` rows, column), threads in that order 64 to a wave; a thread's
    private words go to the staged words where its run ends inside the chunk; at the chunk's end a full wave whose lanes all stand in
    the set adds its lanes' words first -> (words, False where a term was not finite or above the window)"""
    ny, nx = member.shape
    staged, ok, ends = [0] * 5, True, {}
    cols = np.flatnonzero(member.any(axis=0))
    nchunk = -(-ny // rows)
    for k in range(nchunk):
        r0, r1 = k * rows, min((k + 1) * rows, ny)
        for c in cols.tolist():
            acc, live = [0] * 5, False
            for r in range(r0, r1):
                if member[r, c]:
                    t = terms[r, c]
                    live = True
                    if t != 0.0 and t == t:
                        ok = add_private(acc, t, top, defect) and ok
                elif live:
                    staged = [(a + b) % W64 for a, b in zip(staged, acc)]
                    acc, live = [0] * 5, False
            if live:
                ends[k * nx + c] = acc
    mod = (1 << 32) if defect == 'the wave sum in 32 bits' else W64
    for w0 in range(0, nchunk * nx, 64):
        lanes = [ends.get(i) for i in range(w0, w0 + 64)]
        if waves and w0 + 64 <= nchunk * nx and all(a is not None for a in lanes):
            lanes = [[sum(a[j] for a in lanes) % mod for j in range(5)]]
        for a in lanes:
            if a is not None:
                staged = [(x + y) % W64 for x, y in zip(staged, a)]
    return staged, ok


def product(w, g, defect=None):
    with np.errstate(all='ignore'):
        if defect == 'the float32 integrand multiplied in float32' and g.dtype == np.float32:
            return (w.astype(np.float32) * g).astype(np.float64)
        return w * g.astype(np.float64)


def model_tops(c, defect=None):
    bound = SC.bound_over(c['pl']['kept']) if defect == 'the bound over the kept nodes only' else IR.finite_bound
    tops = [list(t) for t in tops_of(c, bound)]
    if defect == 'one window for all slabs':
        tops = [list(tops[0]) for _ in tops]
    if defect == 'one window for all fields':
        tops = [[t[0]] * len(t) for t in tops]
    if defect == 'the tops of fields 4 to 7 from fields 0 to 3':
        tops = [[t[m - 4] if m >= 4 else t[m] for m in range(len(t))] for t in tops]
    return tops


def model(c, defect=None):
    """restatement()'s result by the kernels' route"""
    pl, ns, nlev, kernel = c['pl'], c['nslab'], c['pl']['nlev'], c['kernel']
    ny, nx = pl['ny'], pl['nx']
    tops, nan = model_tops(c, defect), float('nan')
    rows = LR.scan_geometry(ny)[0]
    out = []
    for s in range(ns):
        ws = np.ones((ny, nx)) if c['w'] is None else np.asarray(slab_of(c['w'], s), dtype=np.float64)
        if kernel == 'k21':
            planes = [product(ws, np.asarray(slab_of(g, s)), defect) for g in c['fields']]
        else:
            planes = [ws] + ([] if c['f'] is None else [product(ws, np.asarray(c['f'][s]), defect)])
        if kernel == 'k22':
            keys = sorted(set(zip(np.where(pl['la'] < 0, -1, pl['la']).ravel().tolist(), np.where(pl['lb'] < 0, -1, pl['lb']).ravel().tolist())) - {(-1, -1)})
            res = dict(a=np.array([k[0] for k in keys]), b=np.array([k[1] for k in keys]), n=np.zeros(len(keys), dtype=np.int64),
                       sum_w=np.full(len(keys), nan), sum_wf=np.full(len(keys), nan))
            for i, (a, b) in enumerate(keys):
                member = (np.where(pl['la'] < 0, -1, pl['la']) == a) & (np.where(pl['lb'] < 0, -1, pl['lb']) == b)
                res['n'][i] = int(member.sum())
                for name, plane, top in zip(('sum_w', 'sum_wf'), planes, tops[s]):
                    words, ok = run_words(member, plane, top, rows, defect)
                    res[name][i] = to_double(words, top, defect) if ok else nan
        else:
            t, n = pl['table'], pl['table'].size
            kids = [np.flatnonzero(t['parent'] == p) for p in range(n)]
            if kernel == 'k19':
                res = {k: np.full(n, nan) for k in TR.SUM_FIELDS}
                for (gname, nname), plane, top in zip((('sum_w', 'net_w'), ('sum_wf', 'net_wf')), planes, tops[s]):
                    gross = [run_words(pl['ring_masks'][p], plane, top, ny, defect, waves=False) for p in range(n)]   # K18's walks: a column
                    for p in range(n):
                        if gross[p][1]:
                            net = [(g - sum(gross[q][0][j] for q in kids[p])) % W64 for j, g in enumerate(gross[p][0])]
                            res[gname][p], res[nname][p] = to_double(gross[p][0], top, defect), to_double(net, top, defect)
            else:
                nf = len(planes)
                res = dict(net=np.full((n, nf), nan), gross=np.full((n, nf), nan))
                memo = {}                                                    # (equal planes in equal windows: the same words)
                for m, (plane, top) in enumerate(zip(planes, tops[s])):
                    key = (plane.tobytes(), top)
                    if key not in memo:
                        memo[key] = [run_words(pl['labels'] == p, plane, top, rows, defect) for p in range(n)]
                    net = memo[key]
                    for p in range(n):
                        if net[p][1]:
                            res['net'][p, m] = to_double(net[p][0], top, defect)
                    for q in range(n):
                        sub, todo = [], [q]
                        while todo:
                            p = todo.pop()
                            sub.append(p)
                            todo.extend(kids[p].tolist())
                        if all(net[p][1] for p in sub):
                            if defect == 'gross folded from rounded doubles':
                                g = 0.0
                                for p in sorted(sub):
                                    g += res['net'][p, m]
                                res['gross'][q, m] = g
                            else:
                                res['gross'][q, m] = to_double([sum(net[p][0][j] for p in sub) % W64 for j in range(5)], top, defect)
        out.extend(dict(res) for _ in range(nlev))
    return out


def same_results(a, b):
    return len(a) == len(b) and all(x.keys() == y.keys() and all(
        same(x[k], y[k]) if np.asarray(x[k]).dtype.kind == 'f' else np.array_equal(x[k], y[k]) for k in x) for x, y in zip(a, b))


def report_how(kernel, batch):
    """the one placement the broken models run at (the sound one runs at every placement, on every plane): the waves' sums where the
    kernel has them"""
    if kernel == 'k19':
        return 'lanes' if batch in SC.PLACED_ONCE else 'strided'
    return 'strided' if batch in SC.SPREAD_ONLY else 'full wave'


def host_calls(kernel):
    """-> [(the name of the list, call, whether the broken models run on it)]: every call of the GPU module"""
    out = []
    for batch in SC.batches():
        first = {}
        for how, c, cases, vname, which in batch_calls(kernel, batch):
            if vname != 'f32':                                                # the same float64 terms as f64
                out.append((batch, c, how == report_how(kernel, batch) and first.setdefault(vname, c['pl']) is c['pl']))
    out += [('floor', c, True) for c, _ in floor_calls(kernel)]
    out += [('per slab', c, True) for c, _, _, _ in per_slab_calls(kernel)]
    if kernel == 'k21':
        out += [('per field', per_field_call(rings('chain', 17, 17), nf)[0], True) for nf in (5, 8)]
    if kernel != 'k22':
        out.append(('fold', fold_call(kernel)[0], True))
    pl = floor_planes(kernel)[0]
    out.append(('float32 integrand', float32_call(kernel, pl), True))
    out += [('overflow', overflow_call(kernel, pl, inside), True) for inside in (False, True)]
    out += [('no wrap', c, True) for c, _, _ in no_wrap_calls(kernel)]
    return out


def model_report(kernel):
    """-> (defect -> the calls that fail under it, list name -> the defects it catches, the calls seen); asserts that the sound model is
    the restatement bit for bit on every call"""
    caught, lists, seen = {d: set() for d in DEFECTS if kernel in ONLY.get(d, KERNELS)}, {}, 0
    for name, c, broken in host_calls(kernel):
        ref = restatement(c)
        assert same_results(model(c), ref), c['what']
        lists.setdefault(name, set())
        seen += 1
        if not broken:
            continue
        for d in caught:
            if not same_results(model(c, d), ref):
                caught[d].add(c['what'])
                lists[name].add(d)
    return caught, lists, seen
