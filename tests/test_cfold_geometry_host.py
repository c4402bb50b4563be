"""The planes of cfold_geometry_cases on the CPU -- no GPU: every case IS what its tag says.  The records come from the restatements of
K12 (contour_join_ref, contour_join_periodic_ref), as in test_cfold_host.py; the events from cfold_ref.folds.  Shown per case: the event
list the planes were drawn with; the geometric property that puts the case onto a boundary of K24's launch geometry (a wave or tile
edge between or inside events, full staging slots, the number of chunks of rows and where a fold meets them), worked out from the
crossing flags alone; that the broken rule of cfold_ref.WRONG the case is there for changes its result; and that gap and gap + 1 on the
same planes give different numbers of events."""
import functools

import numpy as np
import pytest

import cfold_geometry_cases as GC
import cfold_ref as FR
import cinside_ref as IR
import contour_join_periodic_ref as JP
import contour_join_ref as JR

CASES = GC.cases()


@functools.lru_cache(maxsize=None)
def records(name):
    case = CASES[name]
    return GC.stacked(case, lambda m: (JP if case.periodic else JR).stack_records(FR.field(m)[None], FR.LEVEL))


@functools.lru_cache(maxsize=None)
def ref(name, wrong=None):
    case = CASES[name]
    return FR.folds(*records(name), *GC.shape(case), case.periodic, case.select, gap=case.gap, ncont=case.ncont, wrong=wrong)


def events_of(out, r):
    a = int(out['event_count'][:r].sum())
    b = a + int(out['event_count'][r])
    return list(zip(out['c_west'][a:b].tolist(), out['c_east'][a:b].tolist(), out['ncol'][a:b].tolist()))


def east(a, b, nx):
    """the columns a, a + 1, .. b going east round the ring"""
    return [(a + d) % nx for d in range((b - a) % nx + 1)]


def test_the_cases_the_issue_of_the_geometry_names_are_all_there():
    tags = [c.tag for c in CASES.values()]
    assert len(set(tags)) >= 25 and all(tags)
    assert max(GC.shape(c)[0] * GC.shape(c)[1] for c in CASES.values()) == 9 * 1000
    assert max(len(c.masks) for c in CASES.values()) == GC.MANY == 300
    rows = [n for n, c in CASES.items() if GC.shape(c)[0] > 9]
    assert all(n.startswith('ny ') for n in rows), rows                      # a plane taller than 9 rows is about rows


@pytest.mark.parametrize('name', sorted(CASES))
def test_the_events_of_every_plane_are_the_ones_it_was_drawn_with(name):
    case, out = CASES[name], ref(name)
    ny, nx = GC.shape(case)
    assert out['event_count'].tolist() == [len(e) for e in case.events]
    for r, drawn in enumerate(case.events):
        assert events_of(out, r) == drawn, (name, r)
        assert [cw for cw, _, _ in drawn] == sorted(cw for cw, _, _ in drawn)                # ordered by c_west, a joined event last
        folded = out['ncross'][r] >= 3
        want = np.full(nx, -1)
        for j, (cw, ce, ncol) in enumerate(drawn):
            cols = [c for c in east(cw, ce, nx) if folded[c]]
            assert len(cols) == ncol and folded[cw] and folded[ce]
            want[cols] = j
        assert np.array_equal(out['col_event'][r], want), (name, r)
        assert (case.masks[r] is not None) or not out['ncross'][r].any()
    assert np.array_equal(out['nodes'].sum(axis=1) > 0, np.ones(len(out['nodes']), dtype=bool))


@pytest.mark.parametrize('name', sorted(CASES))
def test_every_case_lies_on_the_boundary_its_tag_names(name):
    case, out = CASES[name], ref(name)
    ny, nx = GC.shape(case)
    pins = case.pins
    assert pins, name
    ev, label = events_of(out, 0), out['col_event'][0]
    X = IR.crossing_flags(*records(name), ny, nx, case.periodic, case.select)
    geo = IR.scan_geometry(ny, nx, len(case.masks))
    spans = [(int(np.flatnonzero(X[r, :, c])[0]), int(np.flatnonzero(X[r, :, c])[-1]))
             for r in range(X.shape[0]) for c in np.flatnonzero(X[r].sum(axis=0) >= 3)]      # (lo, hi) of every folded column
    for key, v in pins.items():
        if key == 'apart':
            pairs = list(zip(ev[:-1], ev[1:])) + ([(ev[-1], ev[0])] if case.periodic else [])
            between = [east((p[1] + 1) % nx, (q[0] - 1) % nx, nx) for p, q in pairs]
            hit = [b for b in between if v[0] in b and v[1] in b]
            assert len(hit) == 1 and (label[hit[0]] == -1).all() and (out['ncross'][0, hit[0]] < 3).all()
            assert len(hit[0]) > case.gap
        elif key == 'bridged':
            hit = [e for e in ev if v[0] in east(e[0], e[1], nx) and v[1] in east(e[0], e[1], nx)]
            assert len(hit) == 1
            inner = east(v[0], v[1], nx)
            assert (label[inner] == -1).all() and len(inner) <= case.gap
        elif key == 'straddles':
            assert any(cw <= ce and label[cw:v].max() == label[v:ce + 1].max() == j for j, (cw, ce, _) in enumerate(ev) if cw < v <= ce)
        elif key == 'full':
            assert out['event_count'][0] == (nx + 1) // 2 and out['event_count'].size > 1
        elif key == 'wave events':
            waves = [label[a:a + 64] for a in range(0, nx - 63, 64)]
            assert waves and all(np.unique(w[w >= 0]).size == v for w in waves)
        elif key in ('nchunk', 'rc'):
            assert geo[key] == v
        elif key == 'cut':
            assert spans and all(hi // geo['rc'] - (lo + 1) // geo['rc'] + 1 >= v for lo, hi in spans)
        elif key == 'opens':
            assert spans and all((lo + 1) % geo['rc'] == 0 and lo + 1 >= geo['rc'] for lo, hi in spans)
        elif key == 'closes':
            assert spans and all((hi + 1) % geo['rc'] == 0 and hi + 1 <= (geo['nchunk'] - 1) * geo['rc'] for lo, hi in spans)
        elif key == 'ncross':
            assert set(out['ncross_max'].tolist()) == {v} and set(out['ncross'][out['ncross'] >= 3].tolist()) == {v}
        elif key == 'chunk0':
            assert all(int(X[0, :geo['rc'], c].sum()) == v for c in np.flatnonzero(X[0].sum(axis=0) >= 3))
        elif key == 'wrong':
            for wrong in v:
                assert FR.differences(ref(name, wrong), out) != [], (name, wrong)
        elif key == 'next':
            other = CASES[v]
            assert other.gap == case.gap + 1 and all(a is b for a, b in zip(other.masks, case.masks))
            assert ref(v)['event_count'][0] < out['event_count'][0]
        else:
            raise AssertionError('unknown pin %r' % key)


def test_the_seam_events_come_last_and_run_from_the_last_run_into_the_first():
    for name, want in (('empty tiles, ring, gap 109', (900, 10)), ('four runs, ring, gap 2', (297, 2))):
        out = ref(name)
        assert (int(out['c_west'][-1]), int(out['c_east'][-1])) == want and (np.diff(out['c_west']) > 0).all()
        cols = np.flatnonzero(out['col_event'][0] == out['event_count'][0] - 1)
        assert cols.min() < out['c_west'][0] < out['c_west'][-1] <= cols.max()      # the last event holds the first folded column
    plain = ref('four runs, plain, gap 2')
    assert plain['event_count'].tolist() == [4] and plain['c_west'].tolist() == [1, 100, 254, 297]


def test_the_comb_fills_the_slots_of_9_x_513():
    assert ref('comb, plain, nx 513')['event_count'].tolist() == [257, 1] and (513 + 1) // 2 == 257
    assert ref('comb, ring, nx 513')['event_count'].tolist() == [256, 1]
    assert ref('comb, ring, nx 513, gap 1')['event_count'].tolist() == [1, 1]


def test_many_ranges_have_134_events_between_empty_ranges():
    case, out = CASES['many ranges'], ref('many ranges')
    cnt = records('many ranges')[0]
    assert cnt.size == 300 and (cnt[2::3] == 0).all() and (np.delete(cnt, np.s_[2::3]) > 0).all()
    assert out['event_count'].tolist() == [1, 1, 0, 0, 1, 0, 1, 0, 0] * 33 + [1, 1, 0]
    assert out['c_west'].tolist() == ([3, 7, 3, 7] * 34)[:int(out['event_count'].sum())]
