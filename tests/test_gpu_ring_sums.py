"""The sums of K19 (xc_contour_piece_tree_dev: gross and net), K21 (xc_contour_piece_props_dev: net and gross of every field) and K22
(xc_label_overlap_dev: sum_w, sum_wf) at the edges of their windows, BIT FOR BIT against cptree_ref, cpprops_ref and cpoverlap_ref, which
state the header's rule through cinside_ref.window_sum: a window of 160 bits under 2^top, top = 12 + the frexp exponent of the largest
finite |w| (|w f|, |w g_m|) of the slab's WHOLE plane, never below -800, one window per slab and sum (K21: per slab and field); the bits of
a term under 2^(top - 160) cut off toward zero; a NaN term skipped, an infinite one making that sum NaN.  The records suites keep every
term in the middle of its window; here the terms are chosen (ring_sums_cases.py, on the lists of cinside_sums_cases.py): ties, sticky
bits, borrows, every shift against the limb grid, the window's bottom and its floor, a bound that lies in no ring (in the omitted pair, or
in another pair), windows that differ per slab and per field, a float32 integrand, a product that overflows, the largest term a window
admits on every node, and K21's fold of a ring's net words into its ancestors' gross.  Every list runs at four placements -- one column, the
lanes of a row, a stride across waves and chunks, and whole waves in one ring or pair, where the wave adds its lanes' words with shuffles.
test_ring_sums_host.py shows on the CPU that the restatements are the kernels' chain of integer words on these very calls, and which
broken step each list catches.

Every call goes through call / check of the three records suites: guards behind every output, every integer field equal, every sum of
every ring and pair equal bit for bit -- no tolerance anywhere.  K19 and K21 calls are repeated with their records shuffled, K22 calls
with one range per group (cap 1).  The last test is K22's slot counting on many tables of two to eight slots."""
import math

import numpy as np
import pytest

import cinside_sums_cases as SC
import cpiece_records_ref as RR
import cpoverlap_ref as OR
import ring_sums_cases as RC
import test_gpu_cpoverlap_records as T22
import test_gpu_cpprops_records as T21
import test_gpu_cptree_records as T19
from test_gpu_cpinside_records import shuffled

pytestmark = pytest.mark.gpu


def run(ctx, c):
    """one call, checked in full against the restatement in the windows of the bound rule, and repeated -> (per range the dict of
    ring_sums_cases.restatement as the GPU wrote it, the tops)"""
    pl, ns, nlev, what = c['pl'], c['nslab'], c['pl']['nlev'], c['what']
    tops = RC.tops_of(c)
    if c['kernel'] == 'k22':
        la, lb = np.tile(pl['la'], (ns * nlev, 1, 1)), np.tile(pl['lb'], (ns * nlev, 1, 1))
        got, _ = T22.check(ctx, la, lb, nlev, c['w'], c['f'], what=what, tops=tops)
        one, groups = T22.rows(ctx, la, lb, nlev, c['w'], c['f'], cap=1)
        assert groups == ns * nlev and all(a.tobytes() == b.tobytes() for a, b in zip(one, got)), what + ': one range per group'
        return [{k: t[k] for k in OR.DTYPE.names} for t in got], tops
    rec = RC.records(pl, ns)
    geo = (pl['ny'], pl['nx'], pl['periodic'], 0, nlev)
    if c['kernel'] == 'k19':
        got = T19.check(ctx, rec, *geo, what, w=c['w'], f=c['f'], tops=tops)
        again, _ = T19.tables(ctx, shuffled(rec, 7), *geo, w=c['w'], f=c['f'])
        assert T19.same(again, got), what + ': shuffled'
        return [{k: t[k] for k in T19.TR.SUM_FIELDS} for t in got], tops
    tabs, props = T21.check(ctx, rec, *geo, what, w=c['w'], fields=c['fields'], tops=tops)
    t2, p2, _ = T21.results(ctx, shuffled(rec, 7), *geo, w=c['w'], fields=c['fields'])
    assert T19.same(t2, tabs) and T21.same(p2, props), what + ': shuffled'
    return [dict(net=p['net'], gross=p['gross']) for p in props], tops


def top_of(tops, s, column):
    """the top of the window of sum_w ('w') or sum_wf ('f'); ring_sums_cases.as_call gives K21 the two as fields 0 and 1"""
    return tops[s][0 if column == 'w' else 1]


@pytest.mark.parametrize('batch', sorted(SC.batches()))
@pytest.mark.parametrize('kernel', RC.KERNELS)
def test_term_lists_in_w_in_a_float64_f_and_in_a_float32_f_at_every_placement(ctx, kernel, batch):
    """every list of the batch, one per slab: the window is the one the case names, the target's sums (K19 gross and net, K21 gross and net
    of the fields that carry the list, K22 the pair's) are the written-out value, a case about the cut differs from plain fsum, and the
    same list gives the same bits at every placement"""
    bits, hows = {}, set()
    for how, c, cases, vname, which in RC.batch_calls(kernel, batch):
        got, tops = run(ctx, c)
        column = 'w' if vname == 'w' else 'f'
        for j, k in enumerate(which):
            cs, where = cases[k], (c['what'], cases[k]['name'])
            assert tops[j][0 if kernel == 'k21' else 'wf'.index(column)] == cs['top'], where   # (K21: the list is field 0 either way)
            terms = [t for t in RC.list_terms(c, j) if not math.isnan(t)]
            if cs['terms'] is not None:
                assert sorted(t for t in terms if t != 0.0) == sorted(t for t in cs['terms'] if t == t and t != 0.0), where
            sums = RC.target_of(c, got, j, column)                           # (gross, net), or the pair's one sum
            own = ('gross', 'net')
            if cs['background'] != 0.0:                                      # the descendants hold terms too: the net sum alone is the list's
                sums, own = sums[-1:], ('net',)
            if kernel == 'k21' and vname != 'w':                              # fields 2 and 4 (the second pass) hold the list too
                tg = c['pl']['target']
                sums += tuple(float(got[j][key][tg, m]) for key in own for m in (2, 4))
                assert SC.same(got[j]['net'][tg, [1, 3]], [float(c['pl']['inner'].sum())] * 2), where
            if any(math.isinf(t) for t in terms):
                assert all(math.isnan(v) for v in sums), where
                continue
            assert all(SC.same(v, sums[0]) for v in sums), where
            if cs['want'] is not None:
                assert SC.same(sums[0], cs['want']), where
            assert (not SC.same(sums[0], math.fsum(terms))) == cs['cut'], where
            if batch not in SC.PLACED_ONCE:
                key = (vname if vname == 'w' else 'f', cs['name'])           # (a float32 f holds the same float64 terms)
                assert SC.same(sums[0], bits.setdefault(key, sums[0])), where + ('the placement shows',)
        hows.add(how)
    assert hows == ({'strided'} if batch in SC.SPREAD_ONLY else {'lanes', 'full wave'} if batch in SC.PLACED_ONCE else set(RC.PLACEMENTS))


@pytest.mark.parametrize('kernel', RC.KERNELS)
def test_the_floor_of_the_window(ctx, kernel):
    """zero, denormal and NaN weights give +0.0; under a largest weight of 2^-900 the window stands at its floor (top -800, bottom -960):
    the terms at 2^-900 survive whole, a term at 2^-1000 (wholly under the floor) and a denormal product add nothing.  K22: the bound's node lies in the omitted pair and, on the other planes, in the pair (7, 5)"""
    for c, want in RC.floor_calls(kernel):
        got, tops = run(ctx, c)
        assert all(t == -800 for t in np.ravel(tops[0])), c['what']
        if kernel == 'k21':
            tg = c['pl']['target']
            assert SC.same(got[0]['net'][tg], [want['sum_w'], want['sum_wf']]) and SC.same(got[0]['gross'][tg], got[0]['net'][tg]), c['what']
        else:
            assert all(SC.same(v, want['sum_w']) for v in RC.target_of(c, got, 0, 'w')), c['what']
            assert all(SC.same(v, want['sum_wf']) for v in RC.target_of(c, got, 0, 'f')), c['what']


@pytest.mark.parametrize('kernel', RC.KERNELS)
def test_every_slab_has_its_own_windows_and_both_ranges_of_a_slab_use_them(ctx, kernel):
    """two slabs whose bounds differ by 2^60, the sticky tie inside each, two ranges per slab (ncont 2), a shared plane of ones as w with
    a per-slab f: a window taken from the other slab loses the sticky bit or overflows"""
    for c, column, want_tops, want in RC.per_slab_calls(kernel):
        got, tops = run(ctx, c)
        m = 'wf'.index(column)
        for s in range(2):
            assert top_of(tops, s, column) == want_tops[s][m], c['what']
            for r in (2 * s, 2 * s + 1):
                if kernel == 'k21':
                    vals = (got[r]['net'][c['pl']['target'], m], got[r]['gross'][c['pl']['target'], m])
                else:
                    vals = RC.target_of(c, got, r, column)
                assert all(SC.same(v, want[s]) for v in vals), (c['what'], r)


@pytest.mark.parametrize('nf', [5, 8])
def test_k21_has_one_window_per_slab_and_field_in_both_passes_of_the_scan(ctx, nf):
    """the bounds of fields 0, 3, 4 and 7 spread over 2^+-40, rotated slab by slab: the term 2^-110 lies under the floor of the one field
    whose bound is 1.5 2^40 and is lost there alone"""
    c, marked, want_tops, want = RC.per_field_call(RC.rings('chain', 17, 17), nf)
    got, tops = run(ctx, c)
    assert tops == want_tops and marked == [m for m in (0, 3, 4, 7) if m < nf]
    tg = c['pl']['target']
    for s in range(len(marked)):
        assert SC.same(got[s]['net'][tg], want[s]) and SC.same(got[s]['gross'][tg], want[s]), (nf, s)
        assert [m for m in range(nf) if got[s]['net'][tg, m] == 0.0] == [marked[s]]


@pytest.mark.parametrize('kernel', RC.KERNELS)
def test_a_float32_integrand_is_cast_before_the_product_and_an_overflowing_product_lifts_no_window(ctx, kernel):
    for pl in RC.floor_planes(kernel)[:3:2]:
        c = RC.float32_call(kernel, pl)
        w, f = c['w'], (c['fields'][1] if kernel == 'k21' else c['f'])
        got, _ = run(ctx, c)
        m = pl['inner']
        sums = (got[0]['gross'][pl['target'], 1], got[0]['net'][pl['target'], 1]) if kernel == 'k21' else RC.target_of(c, got, 0, 'f')
        net = sums[-1]
        cast_after = (w * f[0].astype(np.float64)).astype(np.float32).astype(np.float64)
        in_float32 = (w.astype(np.float32) * f[0]).astype(np.float64)
        assert f.dtype == np.float32 and SC.same(net, math.fsum((w * f[0].astype(np.float64))[m]))
        assert not SC.same(net, math.fsum(cast_after[m])) and not SC.same(net, math.fsum(in_float32[m]))
        for inside in (False, True):
            c = RC.overflow_call(kernel, pl, inside)
            got, tops = run(ctx, c)
            top_w, top_f = (tops[0][0], tops[0][1])
            assert top_w == 1013 and 0 < top_f <= 53, c['what']                # no window has moved
            if kernel == 'k22':
                assert np.isnan(got[0]['sum_wf']).tolist() == [inside and (a, b) == RC.PAIR for a, b in zip(got[0]['a'], got[0]['b'])]
                assert np.isfinite(got[0]['sum_w']).all() and SC.same(RC.target_of(c, got, 0, 'w')[0], 2.0 ** 1000 if inside else 0.0)
                continue
            t, tg = pl['table'], pl['target']
            up = [tg]
            while t['parent'][up[-1]] >= 0:
                up.append(int(t['parent'][up[-1]]))
            poisoned = np.isin(np.arange(t.size), up) & inside                # the ring and its ancestors, and nothing else
            if kernel == 'k19':
                assert np.isnan(got[0]['sum_wf']).tolist() == poisoned.tolist() and np.isfinite(got[0]['sum_w']).all()
                assert np.isnan(got[0]['net_wf']).tolist() == poisoned.tolist() and np.isfinite(got[0]['net_w']).all()
                assert SC.same(got[0]['net_w'][tg], 2.0 ** 1000 if inside else 0.0)
            else:
                assert np.isnan(got[0]['gross'][:, 1]).tolist() == poisoned.tolist() and np.isfinite(got[0]['gross'][:, 0]).all()
                assert np.isnan(got[0]['net'][:, 1]).tolist() == (np.arange(t.size) == tg).__and__(inside).tolist()
                assert np.isfinite(got[0]['net'][:, 0]).all()


@pytest.mark.parametrize('kernel', RC.KERNELS)
def test_no_word_wraps_when_every_node_holds_the_largest_term_its_window_admits(ctx, kernel):
    """(2 - 2^-52) 2^0 -- all 53 bits set, the bound itself, so at the top of its window -- on every node of one pair of a 70 x 128 plane, of
    the largest ring of a 70 x 128 block plane and of a ring that goes round 128 columns, at both signs: n times the term, rounded once"""
    for c, column, n in RC.no_wrap_calls(kernel):
        got, tops = run(ctx, c)
        assert n > 8000 and (kernel == 'k22') == (n == 70 * 128)
        for s, sign in enumerate((1.0, -1.0)):
            assert top_of(tops, s, column) == 13, c['what']
            want = math.fsum([sign * RC.ALL_ONES] * n)
            if kernel == 'k21':
                m = 'wf'.index(column)
                vals = (got[s]['net'][c['pl']['target'], m], got[s]['gross'][c['pl']['target'], m])
            else:
                vals = RC.target_of(c, got, s, column)
            assert all(SC.same(v, want) for v in vals), (c['what'], sign)


@pytest.mark.parametrize('kernel', ['k19', 'k21'])
def test_the_gross_of_a_parent_is_folded_from_words_not_from_rounded_sums(ctx, kernel):
    """the chain of rings: the child's net is +B, the parent's -B + t, B = (2 - 2^-52) 2^40 and t = (2 - 2^-52) 2^-60.  B is the bound: the
    window's floor is 2^-107 and cuts the last five bits of t.  The parent's gross is that t to the bit -- sums of rounded doubles give 0 --
    and the grandparent's gross the exact sum of all three and its own term, rounded once"""
    c, at, want = RC.fold_call(kernel)
    got, tops = run(ctx, c)
    assert tops[0][0] == 53 and want['t_cut'] == RR.cut(RC.FOLD_T, -107)
    g, n = (got[0]['sum_w'], got[0]['net_w']) if kernel == 'k19' else (got[0]['gross'][:, 0], got[0]['net'][:, 0])
    assert SC.same(n[at['child']], RC.FOLD_B) and SC.same(g[at['child']], RC.FOLD_B)
    assert SC.same(n[at['target']], -RC.FOLD_B) and n[at['child']] + n[at['target']] == 0.0
    assert SC.same(g[at['target']], want['t_cut']), 'the parent gross is t'
    assert SC.same(n[at['parent']], RC.FOLD_G) and SC.same(g[at['parent']], want['parent_gross'])
    assert want['parent_gross'] == math.fsum([RC.FOLD_B, -RC.FOLD_B, want['t_cut'], RC.FOLD_G]) != RC.FOLD_G


# ------------------------------------------------------------------ K22: many small tables
def small_tables():
    """96 ranges (ncont 48, two slabs) of 8 x 9 maps holding 0, 1, 2 or 3 pairs of one run each: tables of 0, 2, 4 and 8 slots, so a wave of 64 slots of
    k_po_count and k_po_emit straddles many ranges; the empty ranges lie in front, in runs in the middle and at the end"""
    rng = np.random.default_rng(2290)
    npair = rng.integers(1, 4, 96)
    npair[[0, 1, 2, 30, 31, 32, 33, 47, 48, 49, 70, 94, 95]] = 0
    la, lb = np.full((96, 8, 9), -1, dtype=np.int32), np.full((96, 8, 9), -1, dtype=np.int32)
    for r, n in enumerate(npair.tolist()):
        for k in range(n):                                                   # pair k: one column, one run
            la[r, 1:7, 3 * k], lb[r, 1:7, 3 * k] = int(rng.integers(0, 50)), 100 + k
    return la, lb, npair, OR.scaled(rng, (2, 8, 9)), OR.scaled(rng, (2, 8, 9), np.float32)


def test_k22_many_tables_of_two_to_eight_slots_with_empty_ones_among_them_under_three_caps(ctx):
    la, lb, npair, w, f = small_tables()
    assert sorted(set(npair.tolist())) == [0, 1, 2, 3] and npair[0] == npair[95] == 0
    got, groups = T22.check(ctx, la, lb, 48, w, f, what='small tables')
    assert groups == 1 and [t.size for t in got] == npair.tolist()
    for cap in (1, 104 * 16):
        again, many = T22.check(ctx, la, lb, 48, w, f, cap=cap, what='small tables, cap %d' % cap)
        assert many > 1 and all(a.tobytes() == b.tobytes() for a, b in zip(again, got)), cap
        if cap == 1:
            assert many == int((npair > 0).sum())
        else:
            assert many < int((npair > 0).sum()), 'a group of sixteen slots holds several ranges'
