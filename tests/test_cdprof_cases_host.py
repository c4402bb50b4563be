"""The cases of cdprof_cases.py on the CPU -- no GPU.  Each HOLDS what test_gpu_cdprof_geometry.py relies on: the constants are the
kernels'; the ramp's distances are exact half-integers and predict_tiles agrees with a count made by hand; every edge set gives the
tile of rows 16 .. 31 the span it is named for; the edge tables have nodes ON their first, last and three inner edges and tiles of
both kinds; every node a test calls NaN, inf, out or cancelling is one; and each deliberately wrong rule -- the two wrong bin rules of
cdprof_ref.RULES, slab 0's weights for every slab, r % ncont as the slab, two fields swapped, another slab's window -- changes the
expected numbers of a named case."""
import bisect
import math
import os
import re

import numpy as np
import pytest

import cdprof_cases as PC
import cdprof_ref as PR
import cinside_ref as CI

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'xcontour_amd', 'csrc')


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_the_constants_are_the_kernels():
    prof, search, sums = source('xc_cdist_profile.h'), source('xc_cdist_search.h'), source('xc_cpiece_sum.h')
    assert re.search(r'constexpr int CDP_SPAN = (\d+);', prof).group(1) == str(PC.SPAN)
    assert re.search(r'constexpr int CDP_EDGES_LDS = (\d+);', prof).group(1) == str(PC.EDGES_LDS)
    assert re.search(r'constexpr int CDP_MAX_EDGES = (\d+);', prof).group(1) == str(PC.MAX_EDGES)
    assert 'constexpr int CDP_MAXCH = 1 + XC_PROPS_MAXF;' in prof
    assert re.search(r'constexpr int CD_T = (\d+);', search).group(1) == str(PC.TILE)
    # the tiles are aligned at node (0, 0): lane t of tile (tr, tc) is node (tr CD_T + t / 16, tc CD_T + t % 16)
    assert 'row = tr * CD_T + (t >> 4), col = tc * CD_T + (t & 15)' in search
    limbs = int(re.search(r'constexpr int CP_L = (\d+);', sums).group(1))
    assert 32 * limbs - 12 == PC.BITS_BELOW
    chunk = int(re.search(r'constexpr int CD_CHUNK = (\d+);', search).group(1))
    # the last word of a full window (16 bins x 9 channels x 5 words behind 512 edges) and the counts behind it end inside the chunk
    assert PC.EDGES_LDS + PC.SPAN * (1 + PC.MAXF) * limbs + PC.SPAN // 2 <= chunk * 5
    assert 'span <= CDP_SPAN' in prof and 'P.nedge <= CDP_EDGES_LDS' in prof


# ------------------------------------------------------------------ the ramp
def test_the_ramp_has_exact_half_integer_distances():
    d = PC.geometry('ramp')['dist']
    rows = np.arange(50.0)
    assert np.array_equal(d[0], np.repeat(np.abs(rows - 0.5)[:, None], 20, axis=1))
    assert np.array_equal(d[1], np.repeat(np.abs(rows - 24.5)[:, None], 20, axis=1))


def hand_count(edges):
    """the ramp's tiles counted with bisect on the rows alone: four tile rows (the last of two rows), two tile columns, two slabs"""
    e = [float(v) for v in edges]
    window = wide = 0
    for level in (0.5, 24.5):
        for r0 in range(0, 50, 16):
            b = []
            for j in range(r0, min(r0 + 16, 50)):
                d = abs(j - level)
                if e[0] <= d <= e[-1]:
                    b.append(len(e) - 2 if d == e[-1] else bisect.bisect_right(e, d) - 1)
            if b:
                span = max(b) - min(b) + 1
                window, wide = window + 2 * (span <= 16), wide + 2 * (span > 16)
    return window, wide


@pytest.mark.parametrize('span,tiles', [(1, (14, 0)), (15, (14, 0)), (16, (14, 0)), (17, (8, 6)), (32, (2, 12))])
def test_predict_tiles_agrees_with_a_hand_count_on_the_ramp(span, tiles):
    """unit edges 0 .. 47: slab 0 (level 0.5) has three tile rows with binned nodes (rows 48, 49 lie beyond 47), slab 1 four, two
    tile columns each: 14 tiles, none wider than 16 bins.  The edge at 20.5 widens the tile rows that hold a distance on both of
    its sides: rows 16 .. 31 of slab 0, rows 0 .. 15 and 32 .. 47 of slab 1 -- 6 tiles."""
    c = PC.case('ramp %d' % span)
    assert PC.predict_tiles(c['dist'], c['edges']) == hand_count(c['edges']) == tiles == PC.expected('ramp %d' % span)['tiles']
    spans = PC.tile_spans(c['dist'], c['edges'])
    assert spans[0, 1, 0] == spans[0, 1, 1] == span                           # the tile the edge set is named for
    if span == 17:
        assert sorted(k for k, v in spans.items() if v > 16) == [(0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 2, 0), (1, 2, 1)]
        assert spans[0, 2, 0] == spans[0, 2, 1] == 16                         # the neighbour stays at 16
    if span == 16:
        assert max(spans.values()) == 16 and (0, 3, 0) not in spans           # a full window; a tile without a binned node
        assert sorted(k for k, v in spans.items() if v == 16) == [(0, 1, 0), (0, 1, 1), (0, 2, 0), (0, 2, 1), (1, 0, 0), (1, 0, 1), (1, 2, 0), (1, 2, 1)]


@pytest.mark.parametrize('name', PC.RAMP + ['smooth'])
def test_the_named_nodes_are_what_they_are_called(name):
    c, e = PC.case(name), PC.expected(name)
    at, f = c['at'], c['fields']
    nslab, N = c['q'].shape[0], c['levels'].shape[-1]
    assert len(f) == 8 and {v.dtype for v in f} == {np.dtype(np.float32), np.dtype(np.float64)} and {v.ndim for v in f} == {2, 3}
    assert np.isnan(f[3][at['nan']]) and np.isnan(f[3]).sum() == 1
    assert np.isposinf(f[4][at['inf']]) and np.isinf(f[4]).sum() == 1
    assert np.isneginf(f[5][(0,) + at['out']]) and np.isinf(f[5]).sum() == 1
    assert f[6][at['zero']] == 0.0 and np.isfinite(c['w']).all()
    for r in range(nslab * N):
        s, k = divmod(r, N)
        bn, bi = PC.bin_of(c, r, at['nan']), PC.bin_of(c, r, at['inf'])
        assert bn >= 0 and bi >= 0, 'the NaN and the inf node lie inside bins'
        assert np.isfinite(e['sums'][s, k, 3]).all()                          # the NaN is skipped
        assert np.flatnonzero(np.isnan(e['sums'][s, k, 4])).tolist() == [bi]  # the inf makes ITS bin NaN
        assert e['flags'][s, k].tolist() == [0, 0, 0, 0, 0, 1, 0, 0, 0]       # set for the inf alone: not the NaN, not the node in no bin
        assert e['nodes'][s, k, bn] > 0 and e['nodes'][s, k, bi] > 0
    for k in range(N):
        assert PC.bin_of(c, k, at['out']) == -1, 'the inf of field 5 lies in no bin'
    assert np.isfinite(e['sums'][:, :, 5]).all() and np.isfinite(e['area']).all()
    assert int(e['nodes'].sum()) < np.isfinite(c['dist']).sum()               # some nodes lie in no bin


@pytest.mark.parametrize('name', ['ramp 15', 'ramp 16', 'ramp 17', 'ramp 32'])
def test_the_cancelling_bins_cancel_and_the_others_do_not(name):
    c, e = PC.case(name), PC.expected(name)
    both = PC.cancelling_bins(e)
    assert both.sum() >= 8 and (e['area'][both] != 0.0).all() and (e['nodes'][both] >= 20).all()
    assert (bits(e['sums'][:, :, 2][both]) == 0).all(), 'exactly +0.0'
    assert (np.abs(c['fields'][2]) >= 1.0).all()                             # every term of the bin is +-2^k w: none is zero
    assert ((e['nodes'] > 0) & (e['sums'][:, :, 2] != 0.0)).sum() >= 8       # the rows that hold +2^k alone
    spans = PC.tile_spans(c['dist'], c['edges'])
    assert both[0, 0, 16:31].any()                                           # in the tile the edge set is named for (rows 16 .. 31)
    assert name != 'ramp 17' or spans[0, 1, 0] > 16


def test_the_infinite_weight_flags_the_area_and_spares_the_field_that_is_zero():
    c, e, base = PC.case('ramp 16 infw'), PC.expected('ramp 16 infw'), PC.expected('ramp 16')
    z = c['at']['zero']
    assert np.isposinf(c['w'][(1,) + z]) and np.isinf(c['w']).sum() == 1 and c['fields'][6][z] == 0.0
    b = PC.bin_of(c, 1, z)
    assert b >= 0
    assert e['flags'][1, 0].tolist() == [1, 1, 1, 1, 1, 1, 1, 0, 1] and np.array_equal(e['flags'][0], base['flags'][0])
    assert np.isnan(e['area'][1, 0, b]) and np.isnan(e['area']).sum() == 1
    with np.errstate(invalid='ignore'):
        terms = (c['w'][1] * c['fields'][6].astype(np.float64))[PR.bins_of(c['dist'][1], c['edges']) == b]
    assert np.isnan(terms).sum() == 1                                         # inf x 0: skipped
    assert np.isfinite(e['sums'][1, 0, 6]).all() and e['sums'][1, 0, 6, b] == math.fsum(terms[~np.isnan(terms)].tolist())
    assert np.array_equal(e['nodes'], base['nodes']) and PR.same_bits(e['sums'][0], base['sums'][0])


def test_without_fields():
    e = PC.expected('ramp 16 nf0')
    assert e['sums'].shape == (2, 1, 0, 47) and e['flags'].shape == (2, 1, 1) and e['tiles'] == (14, 0)
    assert np.array_equal(e['nodes'], PC.expected('ramp 16')['nodes']) and PR.same_bits(e['area'], PC.expected('ramp 16')['area'])


def test_the_smooth_plane_has_tiles_of_both_kinds():
    w, g = PC.expected('smooth')['tiles']
    assert w > 0 and g > 0 and w + g == 27


# ------------------------------------------------------------------ the edge tables
@pytest.mark.parametrize('name', PC.TABLES)
def test_the_edge_tables_hold_nodes_on_their_edges_and_tell_the_bin_rules_apart(name):
    c, e = PC.case(name), PC.expected(name)
    d, edges = c['dist'], c['edges']
    n = int(name.split()[1])
    assert edges.size == n and d.shape[1] * d.shape[2] <= 37 * 45 and (np.diff(edges) > 0.0).all()
    assert edges[0] == d.min() and edges[-1] == d[np.isfinite(d)].max()
    on = PC.on_distances(d)
    assert len(set(on.tolist())) == 3 and np.isin(on, edges).all() and all((d == v).any() for v in on)
    assert e['nodes'][..., 0].sum() > 0 and e['nodes'][..., -1].sum() > 0     # both closed ends hold nodes
    assert int(e['nodes'].sum()) == d.size                                   # ... and no node is left out
    w, g = e['tiles']
    assert w > 0 and g > 0 and w + g == 27, 'a window tile and a global tile (beyond 512 edges both read them from memory)'
    steps = np.diff(edges)
    assert steps.max() > 50.0 * steps.min()                                  # coarse over most of the range, fine in one stretch
    nodes = {rule: PR.profile(d, edges, 3, rule=rule)['nodes'] for rule in PR.RULES}
    assert np.array_equal(nodes['histogram'].reshape(e['nodes'].shape), e['nodes'])
    for rule in PR.RULES[1:]:
        assert not np.array_equal(nodes[rule], nodes['histogram']), rule
    assert nodes['last edge open'][:, -1].sum() < nodes['histogram'][:, -1].sum()
    first = d[d == edges[0]]
    assert (PR.bins_of(first, edges) == 0).all() and (PR.bins_of(first, edges, 'left open') == -1).all()


def test_the_binary_search_takes_its_thirteen_steps_and_ends_on_the_last_edge():
    """4097 edges: lo = 0, hi = 4097 halves thirteen times; a node ON the last edge ends with lo == nedge"""
    c = PC.case('edges 4097')
    assert math.ceil(math.log2(c['edges'].size)) == 13
    d = c['dist']
    assert (PR.bins_of(d[d == c['edges'][-1]], c['edges']) == c['edges'].size - 2).all()


# ------------------------------------------------------------------ the per-slab index
def wrong_rules(c):
    """name -> the expected numbers under a deliberately wrong per-slab rule (sums as (nf, nrange, M))"""
    N = c['levels'].shape[-1]
    f = list(c['fields'])
    swapped = [f[-1]] + f[1:-1] + [f[0]]
    return {'slab 0 weights': PR.profile(c['dist'], c['edges'], N, c['w'][0], f),
            'r % ncont': PC.profile_by_slab(c['dist'], c['edges'], lambda r: r % N, c['w'], f),
            'fields swapped': PR.profile(c['dist'], c['edges'], N, c['w'], swapped)}


@pytest.mark.parametrize('name', ['magnitude', 'ramp 16'])
def test_a_wrong_slab_or_field_gives_other_bits(name):
    c = PC.case(name)
    N = c['levels'].shape[-1]
    right = PR.profile(c['dist'], c['edges'], N, c['w'], c['fields'])
    again = PC.profile_by_slab(c['dist'], c['edges'], lambda r: r // N, c['w'], c['fields'])
    assert all(PR.same_bits(np.nan_to_num(right[k], nan=-1.0), np.nan_to_num(again[k], nan=-1.0)) for k in ('area', 'sums'))
    assert c['w'].ndim == 3 and any(v.ndim == 3 for v in c['fields']) and any(v.ndim == 2 for v in c['fields'])
    for rule, wrong in wrong_rules(c).items():
        assert np.array_equal(wrong['nodes'], right['nodes']), rule             # the counts cannot tell: the sums must
        with np.errstate(invalid='ignore'):
            differs = (bits(wrong['area']) != bits(right['area'])).any() or (bits(wrong['sums']) != bits(right['sums'])).any()
        assert differs, '%s: %s does not tell' % (name, rule)
        if rule != 'fields swapped':                                           # every slab but the one both rules agree on
            per_slab = [m for m, v in enumerate(c['fields']) if v.ndim == 3]
            nr = right['area'].shape[0]
            hit = {r for r in range(nr) if (bits(wrong['area'][r]) != bits(right['area'][r])).any()
                   or (bits(wrong['sums'][per_slab, r]) != bits(right['sums'][per_slab, r])).any()}
            agree = {r for r in range(nr) if (r // N) == (0 if rule == 'slab 0 weights' else r % N)}
            assert hit == set(range(nr)) - agree, rule


def test_another_slabs_window_loses_the_sum_on_the_magnitude_case():
    """the scales lie further apart than the 148 bits the window keeps below its bound: under the top of ANY other slab a slab's terms
    lie above the window (flagged) or lose bits; under its own top every sum is math.fsum's"""
    c = PC.case('magnitude')
    assert c['levels'].shape[-1] == 3 and c['q'].shape[0] == 3
    assert (np.diff(np.log2(c['scales'])) > PC.BITS_BELOW).all()
    ny, nx = c['dist'].shape[1:]
    tops = [CI.window_tops(c['w'], c['fields'][0], 3, ny, nx)[s] for s in range(3)]
    for s in range(3):
        b = PR.bins_of(c['dist'][3 * s + 1], c['edges'])
        k = int(np.bincount(b[b >= 0]).argmax())
        for ch, terms in enumerate((c['w'][s], c['w'][s] * c['fields'][0][s])):
            t = terms[b == k]
            exact = math.fsum(t.tolist())
            assert CI.window_sum(t, tops[s][ch]) == exact != 0.0
            for o in range(3):
                if o != s:
                    above = np.abs(t).max() >= 2.0 ** tops[o][ch]
                    assert above or CI.window_sum(t, tops[o][ch]) != exact, (s, o, ch)


def test_swapping_the_slabs_swaps_the_expected_numbers():
    c = PC.case('magnitude')
    e, s = PC.expected('magnitude'), PC.expected_of(PC.swapped_slabs(c))
    for k in ('nodes', 'area', 'sums', 'flags'):
        assert np.array_equal(bits(s[k]) if s[k].dtype == np.float64 else s[k], (bits(e[k]) if e[k].dtype == np.float64 else e[k])[::-1]), k
    assert not PR.same_bits(s['area'], e['area'])


# ------------------------------------------------------------------ the ring and the plane edges
def test_the_ring_case_has_both_signs_and_three_contour_groups():
    c, e = PC.case('ring'), PC.expected('ring')
    assert c['signed'] and c['select'] == 'main' and c['period'] > 0.0 and c['levels'].size == 3 and c['q'].shape[0] == 2
    assert (c['dist'] < 0).any() and (c['dist'] > 0).any() and c['edges'][0] < 0.0 < c['edges'][-1]
    assert (e['nodes'].sum(axis=-1) == 37 * 40).all() and not PR.same_bits(e['area'][0], e['area'][1])


@pytest.mark.parametrize('name,tiles', zip(PC.PLANES, [(4, 0), (4, 0), (8, 0)]))
def test_the_planes_around_one_tile_column(name, tiles):
    """ny 17: a tile row of 16 rows and one of a single row; nx 15, 16, 17: a tile column short of, equal to and one past a tile"""
    c, e = PC.case(name), PC.expected(name)
    assert e['tiles'] == tiles and c['levels'].size == 2
    assert (e['nodes'].sum(axis=-1) == c['dist'].shape[1] * c['dist'].shape[2]).all() and (e['nodes'] > 0).sum() >= 6
    assert all((r, 1, 0) in PC.tile_spans(c['dist'], c['edges']) for r in range(2))       # the one-row tile row holds binned nodes
