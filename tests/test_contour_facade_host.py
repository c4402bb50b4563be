# -*- coding: utf-8 -*-
"""The facade of the contour methods that run on K12's records -- cal_contour_pieces, cal_contour_overturning,
cal_integral_inside_contours, cal_contour_folds and the six ring methods of `Contour2D` -- pinned without a GPU, over a recording
stand-in for the `Context` methods they call.  Pinned are (1) every positional and keyword argument a method hands to the binding
(arrays with dtype, shape, contiguity and bytes) and everything it returns (names, dims, coordinates, dtypes, nesting, bytes), as
two digests per case; (2) the text of every refusal, and for every pair of refusals of one method which of the two a call with both
defects raises.  The expected values are a recording, tests/golden/contour_facade_host.json, written by
`python tests/test_contour_facade_host.py --record` from the revision before the facade's openings and closings were shared: it
states what that revision did, not what would be tidier.  (3) the argument list `Context.contour_folds` hands to
xc_contour_folds_dev, over the stand-in library of standin_lib.py, like test_host_ring_records.py pins K17's."""
import hashlib
import itertools
import json
import os
import sys
import zlib

import numpy as np
import pytest

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from standin_lib import _K12, _Lib          # noqa: E402

import xcontour_amd as xa                   # noqa: E402
from xcontour_amd import _native as nat     # noqa: E402
from xcontour_amd import labeled as lb      # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'contour_facade_host.json')
NY, NX, N = 5, 7, 3
LEAD = {'L0': ((), ()), 'L23': (('time', 'lev'), (2, 3))}
CTX = nat.Context


# ------------------------------------------------------------------ what a value is, bit for bit
def sig(v):
    if isinstance(v, np.bool_):
        return 'np.bool_:%r' % bool(v)
    if v is None or isinstance(v, (bool, str)):
        return repr(v)
    if isinstance(v, (float, np.floating)):
        return '%s:%s' % (type(v).__name__, float(v).hex())
    if isinstance(v, (int, np.integer)):
        return '%s:%d' % (type(v).__name__, int(v))
    if isinstance(v, np.ndarray):
        if v.dtype.names:
            return {'rec': [[k, str(v.dtype[k])] + [sig(np.ascontiguousarray(v[k]))] for k in v.dtype.names], 'shape': list(v.shape)}
        lay = 'C' if v.flags.c_contiguous else 'F' if v.flags.f_contiguous else '-'
        return '%s%r%s:%s' % (v.dtype.str, tuple(v.shape), lay, hashlib.sha1(np.ascontiguousarray(v).tobytes()).hexdigest())
    if isinstance(v, lb.Dataset):
        return {'dataset': [[k, sig(a)] for k, a in v.items()]}
    if lb.is_labeled(v):
        val, dims, coords, name = lb.unwrap(v)
        return {'name': sig(name), 'dims': list(dims), 'coords': sorted([k, sig(np.asarray(c))] for k, c in coords.items()), 'values': sig(val)}
    if isinstance(v, dict):
        return {'dict': [[k, sig(a)] for k, a in v.items()]}
    if isinstance(v, (list, tuple)):
        return {type(v).__name__: [sig(a) for a in v]}
    if isinstance(v, np.dtype) or isinstance(v, type):
        return 'type:%s' % np.dtype(v).str
    raise TypeError('no signature for %r' % type(v))


def digest(s):
    return hashlib.sha1(json.dumps(s, sort_keys=True).encode()).hexdigest()[:16]


# ------------------------------------------------------------------ the recording stand-in for the Context
def _table(rng, dtype, n):
    out = np.zeros(n, dtype=dtype)
    for k in dtype.names:
        t, shape = dtype[k].base, (n,) + dtype[k].shape
        if t.kind == 'f':
            out[k] = rng.standard_normal(shape)
        elif t.kind == 'b':
            out[k] = rng.random(shape) < 0.5
        else:
            out[k] = rng.integers(0, 40, shape)
    return out


class Recorder(object):
    """the `Context` methods the facade calls: each records its arguments as it got them and returns canned arrays of the
    binding's shapes and dtypes, a function of the method's name and the shapes alone"""
    XC_PROPS_MAXF = CTX.XC_PROPS_MAXF
    OVERTURN_SELECT = CTX.OVERTURN_SELECT

    def __init__(self):
        self.calls = []

    def _take(self, name, args, kw):
        self.calls.append([name, [sig(a) for a in args], sorted([k, sig(v)] for k, v in kw.items())])
        n, ny, nx = args[0].shape
        c = args[2 if name == 'contour_piece_overlap' else 1] if len(args) > 1 else None
        return np.random.default_rng(zlib.crc32(name.encode())), n, ny, nx, c.shape[-1] if isinstance(c, np.ndarray) else c

    @staticmethod
    def _counts(n, ncont, shift=0):
        s, k = np.meshgrid(np.arange(n), np.arange(ncont), indexing='ij')
        return ((s + 2 * k + shift) % 3).astype(np.uint64)

    def minmax(self, q):
        rng, n = self._take('minmax', (q,), {})[:2]
        return np.sort(rng.standard_normal((n, 2)), axis=1)

    def contours(self, q, N, increase, ctr_dtype, **kw):
        rng, n = self._take('contours', (q, N, increase, ctr_dtype), kw)[:2]
        return np.sort(rng.standard_normal((n, int(N))), axis=1).astype(ctr_dtype)

    def contour_pieces(self, q, contours, ycoord, xcoord, **kw):
        rng, n, ny, nx, nc = self._take('contour_pieces', (q, contours, ycoord, xcoord), kw)
        pc = self._counts(n, nc)
        tab = _table(rng, CTX.PIECE_DTYPE, int(pc.sum()))
        rows = np.sort(rng.uniform(0, ny - 1, (tab.size, 2)), axis=1)
        tab['row_min'], tab['row_max'] = rows[:, 0], rows[:, 1]
        return pc, tab

    def _columns(self, rng, n, nc, ny, nx):
        ncross = rng.integers(0, 5, (n, nc, nx)).astype(np.int32)
        rows = np.sort(rng.uniform(0, ny - 1, (2, n, nc, nx)), axis=0)
        rows[:, ncross == 0] = np.nan
        return ncross, rows[0], rows[1]

    def contour_overturning(self, q, contours, **kw):
        rng, n, ny, nx, nc = self._take('contour_overturning', (q, contours), kw)
        return self._columns(rng, n, nc, ny, nx) + (
            rng.integers(0, 4, (n, nc)).astype(np.int32), rng.integers(-1, 60, (n, nc)), rng.integers(0, 30, (n, nc)),
            rng.integers(-1, 2, (n, nc)).astype(np.int32))

    def contour_interior(self, q, contours, **kw):
        rng, n, ny, nx, nc = self._take('contour_interior', (q, contours), kw)
        res = (rng.integers(0, ny * nx, (n, nc)), rng.standard_normal((n, nc)), rng.standard_normal((n, nc)) if kw.get('f') is not None else None)
        return res + ((rng.random((n, nc, ny, nx)) < 0.5,) if kw.get('return_mask') else ())

    def contour_folds(self, q, contours, **kw):
        rng, n, ny, nx, nc = self._take('contour_folds', (q, contours), kw)
        ec = self._counts(n, nc, 1)
        tab = _table(rng, CTX.FOLD_DTYPE, int(ec.sum()))
        for k in ('c_west', 'c_east'):
            tab[k] = rng.integers(0, nx, tab.size)
        rows = np.sort(rng.uniform(0, ny - 1, (tab.size, 2)), axis=1)
        tab['row_lo'], tab['row_hi'] = rows[:, 0], rows[:, 1]
        tab['area'] = np.abs(tab['area'])
        tab['my'] = tab['area'] * rng.uniform(0, ny - 1, (tab.size, 2))
        tab['mx'] = tab['area'] * rng.uniform(0, nx, (tab.size, 2))
        if tab.size > 2:
            tab['area'][0, 1], tab['area'][2, 0] = 0.0, np.nan
        if kw.get('f') is None:
            tab['integral'] = np.nan
        return self._columns(rng, n, nc, ny, nx) + (rng.integers(-1, 3, (n, nc, nx)).astype(np.int32), ec, tab)

    def _rings(self, rng, pc, ny, nx, tree=True):
        tab = _table(rng, CTX.PIECE_TREE_DTYPE if tree else CTX.PIECE_INTERIOR_DTYPE, int(pc.sum()))
        if tree:                                                     # the second ring of a range of two hangs under the first
            second = np.concatenate([np.arange(int(c)) for c in pc.ravel()] or [np.empty(0, dtype=np.int64)]) == 1
            tab['parent'], tab['depth'] = np.where(second, 0, -1), second
        return tab

    def contour_piece_interiors(self, q, contours, **kw):
        rng, n, ny, nx, nc = self._take('contour_piece_interiors', (q, contours), kw)
        pc = self._counts(n, nc)
        return pc, self._rings(rng, pc, ny, nx, tree=False)

    def contour_piece_tree(self, q, contours, **kw):
        rng, n, ny, nx, nc = self._take('contour_piece_tree', (q, contours), kw)
        pc = self._counts(n, nc)
        return pc, self._rings(rng, pc, ny, nx)

    def contour_piece_labels(self, q, contours, **kw):
        rng, n, ny, nx, nc = self._take('contour_piece_labels', (q, contours), kw)
        pc = self._counts(n, nc)
        return pc, self._rings(rng, pc, ny, nx), rng.integers(-1, 2, (n, nc, ny, nx)).astype(np.int32)

    def contour_piece_props(self, q, contours, **kw):
        rng, n, ny, nx, nc = self._take('contour_piece_props', (q, contours), kw)
        pc = self._counts(n, nc)
        tab = self._rings(rng, pc, ny, nx)
        nf, has_x = len(kw.get('fields', ())), kw.get('x') is not None
        pr = {'gross': rng.standard_normal((tab.size, nf)), 'net': rng.standard_normal((tab.size, nf))}
        for k in ('x_min', 'x_max'):
            pr[k] = rng.standard_normal(tab.size) if has_x else None
        for k in ('at_min', 'at_max'):
            pr[k] = rng.integers(-1, ny * nx, tab.size) if has_x else None
        return pc, tab, pr

    def contour_piece_overlap(self, qa, qb, contours, **kw):
        rng, n, ny, nx, nc = self._take('contour_piece_overlap', (qa, qb, contours), kw)
        pc, pcb, pairs = self._counts(n, nc), self._counts(n, nc, 1), self._counts(n, nc, 2)
        return pc, self._rings(rng, pc, ny, nx), pcb, self._rings(rng, pcb, ny, nx), pairs, _table(rng, CTX.OVERLAP_DTYPE, int(pairs.sum()))

    def contour_piece_tracks(self, q, contours, **kw):
        rng, n, ny, nx, nc = self._take('contour_piece_tracks', (q, contours), kw)
        pc, lc, tc = self._counts(n, nc), self._counts(n - 1, nc, 1), self._counts(1, nc, 2)[0]
        lk = _table(rng, CTX.TRACK_LINK_DTYPE, int(lc.sum()))
        lk['step'] = np.repeat(np.arange(n - 1), lc.sum(axis=1).astype(np.int64))
        return (pc, self._rings(rng, pc, ny, nx), _table(rng, CTX.RING_TRACK_DTYPE, int(pc.sum())), lc, lk, tc,
                _table(rng, CTX.PIECE_TRACK_DTYPE, int(tc.sum())))


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(nat, 'default_context', lambda device=0: r)
    return r


# ------------------------------------------------------------------ the inputs
def coords_of(lead, asc, nx=NX):
    names, shape = LEAD[lead]
    lat = np.linspace(-60.0, 60.0, NY) if asc else np.linspace(60.0, -60.0, NY)
    c = {'lat': lat, 'lon': np.arange(nx) * 40.0}
    c.update({d: np.arange(n, dtype=np.float64) * 10 for d, n in zip(names, shape)})
    return names, shape, c


def field(lead, asc, seed, dtype=np.float32, nx=NX, plane=False):
    names, shape, c = coords_of(lead, asc, nx)
    if plane:
        names, shape = (), ()
    v = np.random.default_rng(seed).standard_normal(shape + (NY, nx)).astype(dtype)
    return xa.DataArray(v, names + ('lat', 'lon'), {k: c[k] for k in names + ('lat', 'lon')}, 'pv%d' % seed)


def levels_of(kind, lead, per_time=False):
    if kind == 'int':
        return N
    if kind == 'list':
        return [0.5, float('nan'), -0.5]
    names, shape, c = coords_of(lead, True)
    v = np.empty(shape + (N,))
    for i in np.ndindex(*shape):            # another order of the levels at every `lev` (`per_time`: at every `time` too)
        k = (i[-1] if i else 0) + (i[0] if per_time and i else 0)
        v[i] = np.roll([-0.25, 0.25, 0.75], k) + 0.01 * sum(i)
    cc = dict({d: c[d] for d in names}, contour=np.array([10.0, 20.0, 30.0]))
    return xa.DataArray(v, names + ('contour',), cc, 'levels')


def weights_of(kind, lead):
    nslab = int(np.prod(LEAD[lead][1], dtype=int))
    rng = np.random.default_rng(3)
    return {'A1': rng.uniform(1, 2, NY), 'A2': rng.uniform(1, 2, (NY, NX)), 'A3': rng.uniform(1, 2, (nslab, NY, NX))}[kind]


def obj(lead, asc, dA, nx=NX):
    return xa.Contour2D(field(lead, asc, 1, nx=nx), dA, dims={'X': 'lon', 'Y': 'lat'}, dimEq={'Y': 'lat'}, increase=True, lt=False)


PERIODIC = {'P0': False, 'P1': True, 'Pn': 300.0}
SELECT = {'P0': 'all', 'P1': 'main', 'Pn': 'circumpolar'}
# (periodic, dA, integrand): every pair of values of two of the three occurs once
REST = [('P0', 'A1', 'G0'), ('P0', 'A2', 'G1'), ('P0', 'A3', 'G2'), ('P1', 'A1', 'G1'), ('P1', 'A2', 'G2'), ('P1', 'A3', 'G0'),
        ('Pn', 'A1', 'G2'), ('Pn', 'A2', 'G0'), ('Pn', 'A3', 'G1')]
METHODS = ['cal_contour_pieces', 'cal_contour_overturning', 'cal_integral_inside_contours', 'cal_contour_folds',
           'cal_integral_inside_pieces', 'cal_contour_piece_tree', 'cal_contour_piece_labels', 'cal_contour_piece_props',
           'cal_contour_piece_overlap', 'cal_contour_piece_tracks']
CASES = [(m, lead, lv, co) + r for m in METHODS for lead in LEAD for lv in ('int', 'list', 'lab') for co in ('asc', 'desc') for r in REST
         if not (m == 'cal_contour_piece_tracks' and lead == 'L0')]


def keywords(method, lead, asc, per, dA, g):
    """the keyword arguments of one case: `side`, `select` and the rest ride on the three axes of REST"""
    integrand = {'G0': None, 'G1': field(lead, asc, 2, np.float64), 'G2': field(lead, asc, 4, np.float32, plane=True)}[g]
    side = 'lower' if dA == 'A2' else 'upper'
    kw = {'periodic': PERIODIC[per]}
    if method == 'cal_contour_pieces':
        kw['latlon'] = per == 'P1'
        if per == 'Pn':
            kw['periodic'] = 300.0
        return kw
    if method == 'cal_contour_overturning':
        return dict(kw, select=SELECT[per])
    if method == 'cal_integral_inside_contours':
        return dict(kw, select=SELECT[per], side=side, integrand=integrand, return_mask=per == 'P1')
    if method == 'cal_contour_folds':
        return dict(kw, select=SELECT[per], integrand=integrand, gap=1 if dA == 'A3' else 0)
    kw['side'] = side
    if method == 'cal_contour_piece_props':
        fields = {} if integrand is None else {'u': integrand, 'v': np.random.default_rng(5).standard_normal((NY, NX))}
        extremum = {'P0': None, 'P1': False, 'Pn': field(lead, asc, 6, np.float64)}[per]
        return dict(kw, fields=fields, extremum=extremum, latlon=per == 'P1', centroid=dA != 'A2')
    kw['integrand'] = integrand
    if method == 'cal_contour_piece_overlap':
        kw['other'] = field(lead, asc, 7)
    if method == 'cal_contour_piece_tracks':
        kw.update(along='time', min_overlap=0.25 if dA == 'A3' else 0.0)
    return kw


def run_case(rec, case):
    method, lead, lv, co, per, dA, g = case
    asc = co == 'asc'
    cm = obj(lead, asc, weights_of(dA, lead))
    out = getattr(cm, method)(levels_of(lv, lead), **keywords(method, lead, asc, per, dA, g))
    return [digest(rec.calls), digest(sig(out))]


# ------------------------------------------------------------------ the refusals
def _no_lon(lead='L23'):
    t = field(lead, True, 1)
    return xa.DataArray(t.values, t.dims, {k: v for k, v in t.coords.items() if k != 'lon'}, 'pv')


BASE = {'cal_contour_pieces': dict(latlon=True, periodic=True),
        'cal_contour_overturning': dict(periodic=True, select='main'),
        'cal_integral_inside_contours': dict(periodic=True, select='main', side='upper'),
        'cal_contour_folds': dict(periodic=True, select='main', gap=0)}
for _m in METHODS[4:]:
    BASE[_m] = dict(periodic=True, side='upper')
BASE['cal_contour_piece_overlap']['other'] = field('L23', True, 7)
BASE['cal_contour_piece_tracks']['along'] = 'time'

# a defect: the keywords it overrides; '_dA' / '_nx' change the object, 'contours' the first argument
COMMON = {
    'no coordinate': dict(tracer=_no_lon()),
    'periodic text': dict(periodic='round'),
    'periodic zero': dict(periodic=0.0),
    'periodic against': dict(periodic=-300.0),
    'periodic short': dict(periodic=100.0),
    'two columns': dict(_nx=2),
    'one column': dict(_nx=1),
    'levels type': dict(contours=2.5),
    'levels dim': dict(contours=xa.DataArray(np.zeros(3), ('level',), {}, 'c')),
    'tracer dims': dict(tracer=xa.DataArray(np.zeros((2, 3)), ('lat', 'z'), {'lat': np.arange(2.0), 'lon': np.arange(3.0)}, 'pv')),
}
SELECTED = {'select name': dict(select='most'), 'free edges': dict(periodic=False)}
WEIGHTED = {'dA shape': dict(_dA=np.ones(4)), 'integrand dims': dict(integrand=xa.DataArray(np.zeros((2, 2)), ('a', 'b'), {}, 'g')),
            'integrand plain': dict(integrand=np.zeros((NY, NX)))}
SIDE = {'side name': dict(side='left')}
DEFECTS = {
    'cal_contour_pieces': dict(COMMON, **{'periodic needs latlon': dict(latlon=False)}),
    'cal_contour_overturning': dict(COMMON, **SELECTED),
    'cal_integral_inside_contours': dict(COMMON, **SELECTED, **WEIGHTED, **SIDE),
    'cal_contour_folds': dict(COMMON, **SELECTED, **WEIGHTED, **{'gap type': dict(gap=1.5), 'gap bool': dict(gap=True),
                                                                  'gap negative': dict(gap=-1), 'gap wide': dict(gap=NX)}),
}
for _m in METHODS[4:]:
    DEFECTS[_m] = dict(COMMON, **WEIGHTED, **SIDE)
del DEFECTS['cal_contour_piece_props']['integrand dims'], DEFECTS['cal_contour_piece_props']['integrand plain']
DEFECTS['cal_contour_piece_props'].update({
    'many fields': dict(fields={'f%d' % i: np.zeros((NY, NX)) for i in range(9)}), 'field shape': dict(fields={'u': np.zeros((3, 3))}),
    'field name': dict(fields={'area': np.zeros((NY, NX))})})
DEFECTS['cal_contour_piece_overlap'].update({
    'other plain': dict(other=np.zeros((2, 3, NY, NX))), 'other shape': dict(other=field('L0', True, 7)),
    'other no coordinate': dict(other=_no_lon()), 'other levels': dict(other_contours=np.array([0.5, 0.0, -0.5])),
    'other levels type': dict(other_contours=2.5)})
DEFECTS['cal_contour_piece_tracks'].update({
    'along': dict(along='lat'), 'series order': dict(contours=levels_of('lab', 'L23', per_time=True)),
    'min_overlap': dict(min_overlap=2.0)})


def refusal(method, over):
    """the text a call with the defects `over` is refused with, the exception's type in front; None: it is not refused here"""
    over = dict(over)
    cm = obj('L23', True, over.pop('_dA', np.ones(NY)), nx=over.pop('_nx', NX))
    contours = over.pop('contours', np.array([-0.5, 0.0, 0.5]))
    kw = dict(BASE[method], **over)
    if cm.tracer.shape[-1] != NX and 'other' in kw and 'other' not in over:
        kw['other'] = field('L23', True, 7, nx=cm.tracer.shape[-1])
    try:
        with np.errstate(all='ignore'):
            getattr(cm, method)(contours, **kw)
    except Exception as e:
        return '%s: %s' % (type(e).__name__, e)
    return None


def refusals_of(method):
    d = DEFECTS[method]
    out = {k: refusal(method, v) for k, v in d.items()}
    for a, b in itertools.combinations(sorted(d), 2):
        if not set(d[a]) & set(d[b]):
            out['%s + %s' % (a, b)] = refusal(method, dict(d[a], **d[b]))
    return out


# ------------------------------------------------------------------ the tests
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.mark.parametrize('method', METHODS)
def test_what_reaches_the_binding_and_what_comes_back(rec, method):
    want = golden()['cases']
    bad = []
    for case in CASES:
        if case[0] == method:
            del rec.calls[:]
            with np.errstate(all='ignore'):
                got = run_case(rec, case)
            if got != want['|'.join(case)]:
                bad.append(('|'.join(case), 'arguments' if got[0] != want['|'.join(case)][0] else 'result'))
    assert bad == []


@pytest.mark.parametrize('method', METHODS)
def test_every_refusal_and_which_of_two_comes_first(rec, method):
    want = golden()['refusals'][method]
    got = refusals_of(method)
    assert sorted(got) == sorted(want)
    assert {k: v for k, v in got.items() if v != want[k]} == {}
    # every defect alone is refused by this method or, where the binding refuses it, passes the facade
    assert all(got[k] is not None for k in DEFECTS[method] if k not in ('two columns', 'one column', 'min_overlap')), got


def test_the_inputs_cover_what_they_should():
    """both directions of the equivalent coordinate give both values of `flip` under both sides; every count of the canned tables
    occurs, an empty range included"""
    r = Recorder()
    assert sorted(set(r._counts(6, N).ravel().tolist())) == [0, 1, 2]
    flips = set()
    for co in ('asc', 'desc'):
        for side in ('upper', 'lower'):
            yg = coords_of('L0', co == 'asc')[2]['lat']
            flips.add((co, side, (side == 'upper') != bool(yg[-1] >= yg[0])))
    assert len(flips) == 4 and {f[2] for f in flips} == {False, True}
    assert len(CASES) == 108 * 9 + 54


# ------------------------------------------------------------------ Context.contour_folds -> xc_contour_folds_dev
S, QY, QX, QN, NSEG = 3, 6, 8, 4, 2
CELLS = QY * QX


def D(nbytes, off=0):
    return ('dev', nbytes, off)


@pytest.mark.parametrize('periodic,select,sel', [(False, 'all', 0), (True, 'main', 2)])
@pytest.mark.parametrize('w_per_slab,has_f', [(False, False), (False, True), (True, True)])
def test_the_arguments_of_xc_contour_folds_dev(periodic, select, sel, w_per_slab, has_f):
    ctx = CTX.__new__(CTX)
    ctx.lib, ctx.handle, ctx.device = _Lib(), None, 0
    ctx._buffers, ctx._resident, ctx._staged, ctx._ev_pool = [], {}, [], []
    ctx.max_batch_bytes = 8 << 30
    seg, K24 = _K12[periodic], 'xc_contour_folds_dev'

    def k12(lib, a):                                                # NSEG segments in every range
        if a[9] == 0:
            lib.poke(a[10], np.full(a[3] * a[7], NSEG, dtype=np.uint64))
            return 1
        return 0

    def k24(lib, a):                                                # one event in every range
        if a[20] == 0:
            lib.poke(a[21], np.ones(a[1], dtype=np.uint64))
            return 1
        return 0
    ctx.lib.on = {seg: k12, K24: k24}
    q = np.random.default_rng(7).standard_normal((S, QY, QX))
    w = np.ones((S, QY, QX)) if w_per_slab else np.ones((QY, QX))
    f = np.random.default_rng(8).standard_normal((S, QY, QX)).astype(np.float32) if has_f else None
    res = ctx.contour_folds(q, np.linspace(-1, 1, QN), w=w, f=f, periodic=periodic, select=select, gap=2)
    args = [(name, tuple(ctx.lib.where(v) for v in a)) for name, a in ctx.lib.args]
    assert [name for name, _ in args] == [seg, seg, K24, K24]
    t, ne, R = NSEG * S * QN, S * QN, S * QN
    ins = [S * CELLS * 8 if w_per_slab else CELLS * 8] + ([S * CELLS * 4] if has_f else [])
    dense = [R * QX * 4, R * QX * 8, R * QX * 8, R * QX * 4]
    head = (None, R, D(R * 8), D(t * 8), D(t * 8), D(t * 32), QY, QX, int(periodic), sel, QN, D(ins[0]), int(w_per_slab),
            D(ins[1]) if has_f else None, nat.XC_F32 if has_f else 0, 2) + tuple(D(b) for b in dense)
    assert args[2][1] == head + (0, D(R * 8)) + (None,) * 11
    B = 112 * ne                                                    # an event: seven 8-byte columns, five of them two wide, four 4-byte ones
    E = lambda k: D(B, k * ne)                                      # noqa: E731
    assert args[3][1] == head + (ne, D(R * 8), E(96), E(100), E(104), E(108), E(0), E(8), E(16), E(32), E(48), E(64),
                                 E(80) if has_f else None)
    assert ctx.lib.mallocs == [S * CELLS * 8, QN * 8] + ins + [R * 8] + dense + [R * 8, t * 8, t * 8, t * 32, B]
    assert [v.shape for v in res] == [(S, QN, QX)] * 4 + [(S, QN), (ne,)]
    assert [v.dtype for v in res] == [np.int32, np.float64, np.float64, np.int32, np.uint64, CTX.FOLD_DTYPE]
    assert np.isnan(res[5]['integral']).all() == (not has_f) and ctx._buffers == []


if __name__ == '__main__' and '--record' in sys.argv:
    r = Recorder()
    nat.default_context = lambda device=0: r
    cases = {}
    with np.errstate(all='ignore'):
        for case in CASES:
            del r.calls[:]
            cases['|'.join(case)] = run_case(r, case)
    with open(GOLDEN, 'w') as fh:
        json.dump({'cases': cases, 'refusals': {m: refusals_of(m) for m in METHODS}}, fh, indent=0, sort_keys=True)
        fh.write('\n')
    print('%d cases recorded' % len(cases))
