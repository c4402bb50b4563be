"""The inputs of the K28 geometry tests, shared by test_cdprof_cases_host.py (which shows on the CPU that every case holds what it is
named for and that cdprof_ref tells a wrong rule on exactly these) and test_gpu_cdprof_geometry.py -- a helper, no tests here.

Everything is on the Cartesian plane (radius 0), where the device distance is cdist_ref's bit for bit.  A case is a dict: q
(nslab, ny, nx), levels (N,) or (nslab, N), ycoord, xcoord, period (None: no ring), select, signed, edges, w, fields, and `at`: the
named nodes (row, col) the tests speak of.  The kernel's limits the cases are built around (xc_cdist_profile.h, xc_cdist_search.h,
xc_cpiece_sum.h) are restated below; test_cdprof_cases_host.py reads them out of the headers."""
import functools

import numpy as np

import cdist_cases as CC
import cdist_ref as DR
import cdprof_ref as PR
import contour_join_periodic_ref as JP
import contour_join_ref as JR

TILE = 16                  # CD_T: a workgroup's tile of nodes, aligned at node (0, 0)
SPAN = 16                  # CDP_SPAN: the bins of the LDS window
EDGES_LDS = 512            # CDP_EDGES_LDS: the edges kept in LDS
MAX_EDGES = 4097           # CDP_MAX_EDGES
MAXF = 8                   # XC_PROPS_MAXF
BITS_BELOW = 148           # the bits of the fixed-point window below its bound (CP_L = 5 limbs of 32 bits, 12 above the bound)

SELECT = {'all': 0, 'circumpolar': 1, 'main': 2}


# ------------------------------------------------------------------ the window predictor
def tile_spans(dist, edges):
    """{(range, tile row, tile column): bmax - bmin + 1} of every tile that holds at least one binned node, from the distances alone"""
    dist = np.asarray(dist, dtype=np.float64)
    out = {}
    for r in range(dist.shape[0]):
        b = PR.bins_of(dist[r], edges)
        for tr in range(0, b.shape[0], TILE):
            for tc in range(0, b.shape[1], TILE):
                t = b[tr:tr + TILE, tc:tc + TILE]
                t = t[t >= 0]
                if t.size:
                    out[r, tr // TILE, tc // TILE] = int(t.max()) - int(t.min()) + 1
    return out


def predict_tiles(dist, edges):
    """(tiles_window, tiles_global) as last_cdprofile_profile must report them: a (range, tile) with a binned node takes the window
    when its bins span at most SPAN, else the global words; a tile without a binned node counts in neither"""
    spans = list(tile_spans(dist, edges).values())
    return sum(1 for s in spans if s <= SPAN), sum(1 for s in spans if s > SPAN)


# ------------------------------------------------------------------ weights and fields
def weights(ny, shift=0.0):
    return 1.0 + 0.37 * np.sin(1.0 + shift + np.arange(ny, dtype=np.float64))


def mirror(nx):
    """a factor along x that is the same at columns x and nx - 1 - x, exact in a few bits"""
    x = np.arange(nx)
    return 1.0 + 0.25 * (np.minimum(x, nx - 1 - x) % 3)


def slab_weights(nslab, ny, nx, scales=None):
    """(nslab, ny, nx): the usual profile along y, shifted per slab, times mirror(nx), times an exact power of two per slab"""
    w = np.stack([weights(ny, 3.0 * s)[:, None] * mirror(nx)[None, :] for s in range(nslab)])
    return w if scales is None else w * np.asarray(scales, dtype=np.float64)[:, None, None]


def six_decades(rng, shape):
    return rng.normal(size=shape) * 10.0 ** rng.uniform(0.0, 6.0, size=shape)


def cancelling(ny, nx, seed):
    """+-2^k: column x holds +2^k, column nx - 1 - x holds -2^k (k per row and pair), so under weights that are mirror-symmetric the
    terms of a whole row cancel exactly -- across the tile columns, not inside one.  Every fifth row holds +2^k alone."""
    rng = np.random.default_rng(seed)
    f = np.zeros((ny, nx))
    k = rng.integers(0, 31, size=(ny, nx // 2))
    f[:, :nx // 2] = 2.0 ** k
    f[:, nx - nx // 2:] = -(2.0 ** k)[:, ::-1]
    f[::5] = np.abs(f[::5])
    return f


FIELD_NAMES = ('decades', 'f32 slabs', 'cancel', 'nan', 'inf', 'out', 'zero', 'decades slabs')


def eight_fields(nslab, ny, nx, seed, at):
    """the eight fields, float32 and float64, shared planes and per-slab stacks: 0 mixed signs over six decades; 1 float32 per slab;
    2 +-2^k pairs; 3 a NaN at at['nan']; 4 an inf at at['inf']; 5 per slab, -inf at at['out'] of slab 0 alone; 6 float32, smooth,
    exactly 0 at at['zero']; 7 per slab, six decades -- the last channel of the window"""
    rng = np.random.default_rng(seed)
    fnan = rng.normal(size=(ny, nx)); fnan[at['nan']] = np.nan
    finf = rng.normal(size=(ny, nx)); finf[at['inf']] = np.inf
    fout = rng.normal(size=(nslab, ny, nx)); fout[(0,) + at['out']] = -np.inf
    zero = (1.5 + CC.smooth(ny, nx, seed + 1)).astype(np.float32); zero[at['zero']] = 0.0
    return [six_decades(rng, (ny, nx)), rng.normal(size=(nslab, ny, nx)).astype(np.float32), cancelling(ny, nx, seed + 2), fnan, finf, fout,
            zero, six_decades(rng, (nslab, ny, nx))]


def two_fields(nslab, ny, nx, seed):
    """a shared plane of mixed signs and six decades, and a float32 stack per slab"""
    rng = np.random.default_rng(seed)
    return [six_decades(rng, (ny, nx)), np.stack([CC.smooth(ny, nx, seed + 1 + s) for s in range(nslab)]).astype(np.float32)]


# ------------------------------------------------------------------ the planes and their distances
@functools.lru_cache(maxsize=None)
def geometry(name):
    """name -> dict(q, levels, ycoord, xcoord, period, select, signed, dist): the plane of a family of cases and its reference
    distances (nslab * N, ny, nx), computed once per process and left unchanged"""
    period, select, signed = None, 'all', False
    if name == 'ramp':                                        # q[y, x] = y: the distance of row j to the level k + 0.5 is |j - (k + 0.5)|
        ny, nx = 50, 20
        q = np.repeat(np.repeat(np.arange(ny, dtype=np.float64)[:, None], nx, axis=1)[None], 2, axis=0)
        lv = np.array([[0.5], [24.5]])
        y, x = np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64)
    elif name == 'smooth':                                    # cdist_cases.smooth, 37 x 45, three levels (test_gpu_cdprof.cartesian's)
        ny, nx = 37, 45
        q = CC.smooth(ny, nx, 21 + nx)[None]
        lv = np.array([-0.2, 0.05, 0.35])
        y, x = np.linspace(-30.0, 40.0, ny), np.linspace(0.0, 690.0, nx) + 3.0
    elif name == 'magnitude':                                 # three slabs, three levels each: r / ncont != r
        ny, nx = 33, 40
        q = np.stack([CC.smooth(ny, nx, 50 + s) for s in range(3)])
        lv = np.array([-0.3, 0.0, 0.3])
        y, x, _ = CC.coords(ny, nx, 133)
    elif name == 'ring':                                      # two slabs on the ring of columns, the main ring, signed
        ny, nx = 37, 40
        q = np.stack([CC.ring_field(), np.roll(CC.ring_field(), 7, axis=1)])
        lv = np.array([0.0, 1.0, 2.0])
        y, x, period = CC.coords(ny, nx, 103, periodic=True)
        select, signed = 'main', True
    else:                                                     # '17x15', '17x16', '17x17': one tile row of 16 and one of 1 row
        ny, nx = [int(v) for v in name.split('x')]
        q = CC.smooth(ny, nx, ny * nx)[None]
        lv = np.array([-0.3, 0.2])
        y, x, _ = CC.coords(ny, nx, 100 + nx)
    ring = period is not None
    rec = (JP if ring else JR).stack_records(q, lv)
    dist = PR.distances(rec, ny, nx, ring, SELECT[select], y, x, period if ring else 0.0, signed=signed)
    dist.setflags(write=False)
    return dict(q=q, levels=lv, ycoord=y, xcoord=x, period=period, select=select, signed=signed, dist=dist, rec=rec)


def on_distances(dist):
    """three distances that occur, as test_gpu_cdprof's `on`"""
    fin = np.sort(dist[np.isfinite(dist)])
    return fin[[fin.size // 7, fin.size // 3, (2 * fin.size) // 3]]


def edge_table(n, dist, stretch):
    """n edges from the smallest to the largest finite distance, both ON them: nine evenly spaced, three ON distances that occur, and
    the rest evenly inside `stretch` = (a, b), fractions of the range -- coarse over most of the range, fine in one stretch"""
    fin = dist[np.isfinite(dist)]
    lo, hi = float(fin.min()), float(fin.max())
    base = np.unique(np.r_[np.linspace(lo, hi, 9), on_distances(dist)])
    k = n - base.size
    a, b = lo + stretch[0] * (hi - lo), lo + stretch[1] * (hi - lo)
    e = np.unique(np.r_[base, a + (b - a) * np.arange(1, k + 1) / (k + 1.0)])
    assert e.size == n and e[0] == lo and e[-1] == hi
    return e


#: the ramp's edges by the span they give the tile of rows 16 .. 31 of slab 0 (distances 15.5 .. 30.5).  All end at 47 or below, so
#: rows 48 and 49 of slab 0 (47.5, 48.5) lie in no bin.
RAMP_EDGES = {
    1: np.array([0.0, 15.0, 31.0, 47.0]),
    15: np.delete(np.arange(48.0), 20),                                   # bins 19 and 20 joined
    16: np.arange(48.0),
    17: np.sort(np.r_[np.arange(48.0), 20.5]),                            # one edge more, ON the distance of row 21
    32: np.sort(np.r_[np.arange(0.0, 47.5, 0.5), 20.25]),                 # half bins give 31, one edge more 32
}
RAMP_AT = {'nan': (20, 7), 'inf': (30, 3), 'out': (49, 5), 'zero': (22, 9)}


@functools.lru_cache(maxsize=None)
def case(name):
    """name -> the case (geometry(...) with edges, w, fields, at), made once per process"""
    if name.startswith('ramp'):
        g = geometry('ramp')
        part = name.split()
        w = slab_weights(2, 50, 20)
        fields = eight_fields(2, 50, 20, 11, RAMP_AT)
        if 'nf0' in part:
            fields = []
        if 'infw' in part:                                    # an infinite weight in slab 1 alone, where field 6 is 0
            w[(1,) + RAMP_AT['zero']] = np.inf
        return dict(g, edges=RAMP_EDGES[int(part[1])], w=w, fields=fields, at=RAMP_AT)
    if name == 'smooth':
        g = geometry('smooth')
        d = g['dist']
        far = np.unravel_index(d.min(axis=0).argmax(), d.shape[1:])          # the node farthest from all three contours
        top = 0.9 * float(d.min(axis=0)[far])
        near = np.unravel_index(d.max(axis=0).argmin(), d.shape[1:])
        at = {'nan': (11, 13), 'inf': (20, 7), 'out': tuple(int(v) for v in far), 'zero': tuple(int(v) for v in near)}
        on = on_distances(d[d < top])
        edges = np.unique(np.r_[np.linspace(0.0, top, 18), on])
        return dict(g, edges=edges, w=slab_weights(1, 37, 45), fields=eight_fields(1, 37, 45, 12, at), at=at)
    if name.startswith('edges'):
        g = geometry('smooth')
        n = int(name.split()[1])
        return dict(g, edges=edge_table(n, g['dist'], (0.55, 0.6)), w=slab_weights(1, 37, 45)[0], fields=two_fields(1, 37, 45, 5), at={})
    if name == 'magnitude':
        g = geometry('magnitude')
        scales = 2.0 ** np.array([-150.0, 0.0, 150.0])
        rng = np.random.default_rng(14)
        fields = [six_decades(rng, (3, 33, 40)) * scales[:, None, None], CC.smooth(33, 40, 15).astype(np.float32),
                  rng.normal(size=(3, 33, 40)).astype(np.float32)]
        d = g['dist']
        edges = np.unique(np.r_[np.linspace(0.0, float(d.max()), 9), on_distances(d)])
        return dict(g, edges=edges, w=slab_weights(3, 33, 40, scales), fields=fields, at={}, scales=scales)
    g = geometry(name)
    d = g['dist']
    ny, nx = d.shape[1:]
    lo = float(d.min()) if g['signed'] else 0.0
    edges = np.unique(np.r_[np.linspace(lo, float(d.max()), 9), on_distances(d)])
    nslab = g['q'].shape[0]
    return dict(g, edges=edges, w=slab_weights(nslab, ny, nx)[0], fields=two_fields(nslab, ny, nx, 16 + nx), at={})


RAMP = ['ramp %d' % s for s in sorted(RAMP_EDGES)]
TABLES = ['edges 512', 'edges 513', 'edges 4097']
PLANES = ['17x15', '17x16', '17x17']
ALL = RAMP + ['ramp 16 nf0', 'ramp 16 infw', 'smooth'] + TABLES + ['magnitude', 'ring'] + PLANES


def swapped_slabs(c):
    """the same case with the slab axis of every input reversed"""
    def rev(a):
        return a if a is None else np.ascontiguousarray(a[::-1])
    out = dict(c, q=rev(c['q']), levels=rev(c['levels']) if c['levels'].ndim == 2 else c['levels'],
               w=rev(c['w']) if np.ndim(c['w']) == 3 else c['w'], fields=[rev(f) if f.ndim == 3 else f for f in c['fields']])
    nslab, N = c['q'].shape[0], c['levels'].shape[-1]
    out['dist'] = np.ascontiguousarray(c['dist'].reshape((nslab, N) + c['dist'].shape[1:])[::-1]).reshape(c['dist'].shape)
    return out


# ------------------------------------------------------------------ the expected numbers
def profile_by_slab(dist, edges, slab_of, w, fields, rule='histogram'):
    """cdprof_ref.profile with the slab of range r given by slab_of(r): the right one is r // ncont"""
    parts = []
    for r in range(dist.shape[0]):
        s = slab_of(r)
        parts.append(PR.profile(dist[r:r + 1], edges, 1, w[s] if np.ndim(w) == 3 else w, [f[s] if f.ndim == 3 else f for f in fields], rule))
    return {k: np.concatenate([p[k] for p in parts], axis=0 if k != 'sums' else 1) for k in ('nodes', 'area', 'sums')}


def predict_flags(dist, edges, ncont, w, fields):
    """int32 (nrange, 1 + nf): 1 where a term of that channel of that range, at a node that lies in a bin, is infinite -- the rule of
    include/xcontour_hip.h, K28 section.  A NaN term sets nothing, and neither does a node that lies in no bin."""
    nr = dist.shape[0]
    out = np.zeros((nr, 1 + len(fields)), dtype=np.int32)
    for r in range(nr):
        s = r // ncont
        at = PR.bins_of(dist[r], edges) >= 0
        ws = np.ones(dist.shape[1:]) if w is None else np.asarray(w[s] if np.ndim(w) == 3 else w, dtype=np.float64)
        out[r, 0] = np.isinf(ws[at]).any()
        for m, f in enumerate(fields):
            with np.errstate(invalid='ignore'):
                out[r, 1 + m] = np.isinf((ws * np.asarray(f[s] if f.ndim == 3 else f).astype(np.float64))[at]).any()
    return out


def expected_of(c, rule='histogram'):
    """what Context.contour_distance_profile must return for a case, in its shapes: dict(nodes (nslab, N, M), area, sums
    (nslab, N, nf, M), flags (nslab, N, 1 + nf), tiles: predict_tiles)"""
    nslab, N = c['q'].shape[0], c['levels'].shape[-1]
    M, nf = len(c['edges']) - 1, len(c['fields'])
    ref = PR.profile(c['dist'], c['edges'], N, c['w'], c['fields'], rule)
    out = dict(nodes=ref['nodes'].reshape(nslab, N, M), area=ref['area'].reshape(nslab, N, M),
               sums=np.ascontiguousarray(np.moveaxis(ref['sums'].reshape(nf, nslab, N, M), 0, 2)),
               flags=predict_flags(c['dist'], c['edges'], N, c['w'], c['fields']).reshape(nslab, N, 1 + nf),
               tiles=predict_tiles(c['dist'], c['edges']))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """expected_of(case(name)), computed once per process (read-only: the tests share it)"""
    return expected_of(case(name))


def cancelling_bins(e):
    """bool (nslab, N, M): the bins with nodes whose sum of field 2 (the +-2^k pairs) is exactly +0.0 in the expected numbers"""
    return (e['nodes'] > 0) & (np.ascontiguousarray(e['sums'][:, :, 2]).view(np.int64) == 0)


def bin_of(c, r, node):
    """the bin of a node (row, col) in range r, -1 for none"""
    return int(PR.bins_of(c['dist'][r][node], c['edges']))
