"""K15 (xc_cline.hip, xc_contour_line_integrals) at every launch geometry and kernel instantiation, and its two fixed-point sums bit
for bit.

K15 is the one kernel that puts SIGNED terms through the order-free fixed-point sums: two's-complement chunks, a signed limb fold, the
second channel of k_det3_reduce, a window of its own per slab.  What a wrong fold would do -- a lost borrow, a negative low chunk
rounded the wrong way under the window, a window one exponent off -- lies many orders of magnitude under the 1e-12 sum |term| bar of
test_gpu_cline.py, so here the integral is held to the model cline_ref.det_integrals BIT FOR BIT on inputs whose terms are exact
(cline_ref.fixed_point_case), and to identities that need no model (F -> -F, F -> 2^k F, F = -1).

Every row asserts the record of xc_last_clen_geometry against clength_ref.launch_geometry (K15: 10 LDS words and 16383 cells per copy)
before it looks at results.  Against the numpy restatement (cline_ref.stack) the bars are test_gpu_cline.py's: counts and NaN pattern
exact, lengths 1e-12 relative, integrals 1e-12 of sum |term|.  A level's results must not depend on the other levels of the call, the
LDS copies, the level groups, the blocks per slab or the other slabs."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import clength_ref as CR
import clength_periodic_ref as PR
import cline_ref as LR
from gpu_common import same_bits
from test_gpu_clen_variants import EDGE_X, EDGE_Y, PROBE, coords, field, levels_in, probe_set

pytestmark = pytest.mark.gpu

PERIOD_LL = float(np.float64(np.deg2rad(np.float32(360.0))))


# ------------------------------------------------------------------------------------------------------------------- helpers
def run(ctx, q, F, lv, y, x, latlon=False, period=None, want=None):
    """one call; asserts the launch record against the model (and the pinned fields of `want`) -> (integral, length, nseg, record)"""
    integ, length, nseg = ctx.contour_line_integrals(q, F, lv, y, x, radius=CR.RADIUS if latlon else 0.0, period=period)
    g = ctx.last_clen_geometry()
    S, ny, nx = q.shape
    exp = CR.launch_geometry(np.shape(lv)[-1], ny, nx, S, words=10, copy_cells=16383, wrap=period is not None)
    exp.update(q_dtype=np.dtype(q.dtype), latlon=int(latlon))
    for k, v in exp.items():
        assert g[k] == v, 'record %s: %r, expected %r' % (k, g[k], v)
    for k, v in (want or {}).items():
        assert g[k] == v, 'record %s: %r, pinned %r' % (k, g[k], v)
    print('geometry: ncopy %d ngroup %d bps %d rule %s ntile %d' % (g['ncopy'], g['ngroup'], g['bps'], g['bps_rule'], g['ntile']))
    return integ, length, nseg.astype(np.int64), g


def check(got, ref, what=''):
    """against the restatement, at the bars of test_gpu_cline.py"""
    integ, length, nseg = got[:3]
    r_int, r_len, r_n, r_scale = ref
    assert np.array_equal(nseg, r_n), '%s: counts' % what
    assert np.array_equal(np.isnan(length), np.isnan(r_len)), '%s: length NaN pattern' % what
    assert np.array_equal(np.isnan(integ), np.isnan(r_int)), '%s: integral NaN pattern' % what
    ok = ~np.isnan(r_len)
    if ok.any():
        e = np.abs(length[ok] - r_len[ok]) / np.abs(r_len[ok])
        assert e.max() <= 1e-12, '%s: length rel %.3g' % (what, e.max())
    ok = ~np.isnan(r_int) & (r_scale > 0)
    if ok.any():
        e = np.max(np.abs(integ[ok] - r_int[ok]) / r_scale[ok])
        print('%s: integral error / sum |term| = %.3g' % (what, e))
        assert e <= 1e-12, '%s: integral %.3g of sum |term|' % (what, e)
    zero = ~np.isnan(r_int) & (r_scale == 0)
    assert (integ[zero] == 0).all(), '%s: a sum of zero terms' % what


def same3(a, b, what=''):
    same_bits(a[0], b[0], what + ' integral'); same_bits(a[1], b[1], what + ' length')
    assert np.array_equal(a[2], b[2]), what + ' counts'


def noisy(shape, seed, dt=np.float64):
    """an integrand that differs on every node: both signs, magnitudes over ~2^-4 .. 2^6"""
    rng = np.random.default_rng(1000 + seed)
    return ((1.0 + 3.0 * rng.standard_normal(shape)) * 2.0 ** rng.uniform(-4.0, 4.0, shape)).astype(dt)


def ref_stack(planes, Fs, index, lv, y, x, latlon=False, period=None):
    """the restatement per DISTINCT (plane, integrand) pair (slab s is pair index[s]) -> the four arrays stacked"""
    per_slab = np.ndim(lv) == 2
    cache, out = {}, []
    for s, p in enumerate(index):
        key = (p, s if per_slab else -1)
        if key not in cache:
            cache[key] = LR.stack(planes[p][None].astype(np.float64), Fs[p][None].astype(np.float64), lv[s] if per_slab else lv, y, x,
                                  latlon, period)
        out.append(cache[key])
    return tuple(np.concatenate([o[i] for o in out]) for i in range(4))


# ------------------------------------------------------------------------------------------------------------------- (a) the signed sum
FP_ROWS = [(p, ax, np.float64) for p in LR.FP_PROFILES for ax in (True, False)] + [('mixed', True, np.float32), ('wide', False, np.float32)]


@pytest.mark.parametrize('profile,along_x,tf', FP_ROWS, ids=['%s-%s-%s' % (p, 'x' if a else 'y', np.dtype(t).name) for p, a, t in FP_ROWS])
def test_signed_fixed_point_sum_bit_for_bit(ctx, profile, along_x, tf):
    """cline_ref.fixed_point_case: every segment lies on a grid line (its length one spacing, exactly: the premise of K10's
    test_fixed_point_rule_bit_for_bit) and the integrand varies only along the segments, so F(u) is a node value and every term is
    (0.5 (Fa + Fb)) d: three correctly rounded operations on exact inputs (premise asserted on the CPU).  Integral and length must
    then be the model det_integrals bit for bit.  'cancel': the residue lies 2^40 under sum |term|; 'wide': terms of both signs drop
    their low chunk under the window -- the model differs from the restatement's float sum there; 'under': every term lies under the
    window of a lone node of 1e200: the integral is exactly +0.0 where the length is a number (so neither of these two can meet the
    1e-12 bar against the float sum: they are held to the model alone)"""
    q, F, lv, y, x = LR.fixed_point_case(profile, along_x, tf)
    for s in range(2):
        assert LR.check_fixed_point_premise(q[s], F[s], lv, y, x) > 1000
    got = run(ctx, q, F, lv, y, x, want=dict(ncopy=8, ngroup=1))
    ref = LR.stack(q, F.astype(np.float64), lv, y, x)
    assert np.array_equal(got[2], ref[2])
    assert np.array_equal(np.isnan(got[0]), np.isnan(ref[0])) and np.array_equal(np.isnan(got[1]), np.isnan(ref[1]))
    model = [LR.det_integrals(q[s], F[s], lv, y, x, f_dtype=tf) for s in range(2)]
    m_int, m_len = np.stack([m[0] for m in model]), np.stack([m[1] for m in model])
    same_bits(got[1], m_len, profile + ' length')
    same_bits(got[0], m_int, profile + ' integral')
    ok = ~np.isnan(m_int)
    assert ok.sum() > 40
    if profile in ('wide', 'under'):
        assert (m_int[ok] != ref[0][ok]).all(), 'the window must cost every term bits'
        if profile == 'under':
            assert (got[0][ok] == 0).all() and not np.signbit(got[0][ok]).any()
        check((ref[0], got[1], got[2]), ref, profile)                        # (lengths and counts at the usual bars)
    else:
        check(got, ref, profile)
    if profile == 'cancel':
        assert np.all(np.abs(ref[0][ok]) < 2.0 ** -40 * ref[3][ok]) and (got[0][ok] != 0).all()


# ------------------------------------------------------------------------------------------------------------------- (b) identities
@pytest.fixture(scope='module')
def plane3():
    ny, nx = 67, 131
    q = np.stack([field(ny, nx, seed=s) for s in (31, 32, 33)])
    return q, noisy(q.shape, 1), levels_in(q, 29, seed=3)


@pytest.mark.parametrize('latlon', [False, True])
@pytest.mark.parametrize('tf', [np.float64, np.float32])
def test_minus_one_gives_minus_the_length(ctx, plane3, tf, latlon):
    q, _, lv = plane3
    y, x = coords('hashed', q.shape[1], q.shape[2], latlon, salt=1)
    integ, length, nseg, _ = run(ctx, q, np.full(q.shape, -1.0, dtype=tf), lv, y, x, latlon)
    klen, kn = ctx.contour_lengths(q, lv, y, x, radius=CR.RADIUS if latlon else 0.0)
    assert (nseg > 0).mean() > 0.75
    same_bits(length, klen, 'length is K10\'s'); assert np.array_equal(nseg, kn.astype(np.int64))
    same_bits(integ, -length, 'F = -1')


@pytest.mark.parametrize('latlon', [False, True])
def test_negated_and_scaled_integrand(ctx, plane3, latlon):
    """F -> -F: every chunk negated, every sum negated exactly.  F -> 2^k F: the window moves by k, the chunks do not change"""
    q, F, lv = plane3
    y, x = coords('stretched', q.shape[1], q.shape[2], latlon, salt=2)
    a = run(ctx, q, F, lv, y, x, latlon)
    check(a, LR.stack(q, F, lv, y, x, latlon), 'noisy')
    ok = ~np.isnan(a[0])
    assert ok.mean() > 0.75 and (a[0][ok] != 0).all()
    b = run(ctx, q, -F, lv, y, x, latlon)
    same_bits(b[0], -a[0], 'F -> -F'); same_bits(b[1], a[1], 'length'); assert np.array_equal(a[2], b[2])
    for k in (-200, 37, 300):
        c = run(ctx, q, np.ldexp(F, k), lv, y, x, latlon)
        same_bits(c[0], np.ldexp(a[0], k), 'F -> 2^%d F' % k); same_bits(c[1], a[1], 'length'); assert np.array_equal(a[2], c[2])


def test_slabs_with_windows_at_their_edges(ctx, plane3):
    """between ordinary slabs: an all-NaN integrand (no finite value: bound 0, the floor window; every segment skipped), an all-zero one
    (the floor window again; every term +0) and one of +-1.7e308 (bound x max |F| overflows: the window top is the infinite bound's;
    F(u) + F(v) overflows or the interpolation does: every level that has a segment is NaN)"""
    q3, F3, lv = plane3
    rng = np.random.default_rng(8)
    huge = np.where(rng.random(q3[0].shape) < 0.5, -1.7e308, 1.7e308)
    q = np.stack([q3[0], q3[1], q3[1], q3[2], q3[0], q3[2]])
    F = np.stack([F3[0], np.full_like(F3[0], np.nan), F3[1], np.zeros_like(F3[0]), huge, F3[2]])
    y, x = coords('hashed', q.shape[1], q.shape[2], False, salt=4)
    got = run(ctx, q, F, lv, y, x)
    ref = LR.stack(q, F, lv, y, x)
    check(got, ref, 'six slabs')
    klen, kn = ctx.contour_lengths(q, lv, y, x)
    assert (got[2][1] == 0).all() and np.isnan(got[0][1]).all() and np.isnan(got[1][1]).all() and (kn[1] > 0).any()
    fin = ~np.isnan(got[1][3])
    assert fin.mean() > 0.75 and (got[0][3][fin] == 0).all() and not np.signbit(got[0][3][fin]).any() and np.isnan(got[0][3][~fin]).all()
    same_bits(got[1][3], klen[3], 'zero slab length')
    assert np.isnan(got[0][4]).all() and (~np.isnan(got[1][4])).mean() > 0.75
    same_bits(got[1][4], klen[4], 'huge slab length'); assert np.array_equal(got[2][4], kn[4].astype(np.int64))
    alone = run(ctx, np.ascontiguousarray(q[[0, 2, 5]]), np.ascontiguousarray(F[[0, 2, 5]]), lv, y, x)
    same3([v[[0, 2, 5]] for v in got[:3]], alone, 'neighbours')
    for s in (1, 3, 4):
        one = run(ctx, q[s:s + 1], F[s:s + 1], lv, y, x)
        same3([v[s:s + 1] for v in got[:3]], one, 'slab %d alone' % s)


# ------------------------------------------------------------------------------------------------------------------- (c) copies, groups
GEOM = [(72, 8, 1), (73, 4, 1), (142, 4, 1), (143, 2, 1), (279, 2, 1), (280, 1, 1), (533, 1, 1), (534, 1, 2), (1067, 1, 3)]


@pytest.fixture(scope='module')
def probe_plane():
    ny, nx = 41, 75
    q = np.stack([field(ny, nx, seed=11), field(ny, nx, seed=12)[::-1]])
    y, x = coords('hashed', ny, nx, False, salt=9)
    return q, noisy(q.shape, 2), y, x


@pytest.fixture(scope='module')
def probe_alone(ctx, probe_plane):
    q, F, y, x = probe_plane
    got = run(ctx, q, F, PROBE, y, x, want=dict(ncopy=8, ngroup=1))
    check(got, LR.stack(q, F, PROBE, y, x), 'probe alone')
    assert (got[2] > 0).all()
    return got[:3]


@pytest.mark.parametrize('N,ncopy,ngroup', GEOM, ids=['N%d' % g[0] for g in GEOM])
def test_lds_copies_and_level_groups(ctx, probe_plane, probe_alone, N, ncopy, ngroup):
    q, F, y, x = probe_plane
    lv = probe_set(N, N)
    got = run(ctx, q, F, lv, y, x, want=dict(ncopy=ncopy, ngroup=ngroup, G=min(N, 533)))
    check(got, LR.stack(q, F, lv, y, x), 'N=%d' % N)
    at = np.searchsorted(lv, PROBE)
    same3([v[:, at] for v in got[:3]], probe_alone, 'probe levels among %d' % N)
    if N in (73, 534, 1067):                                              # per-slab levels, across the group split where there is one
        lv2 = np.stack([lv, probe_set(N, N + 1)])
        g2 = run(ctx, q, F, lv2, y, x, want=dict(ncopy=ncopy, ngroup=ngroup))
        check(g2, LR.stack(q, F, lv2, y, x), 'N=%d per slab' % N)
        same3([v[0] for v in g2[:3]], [v[0] for v in got[:3]], 'slab 0')
        at2 = np.searchsorted(lv2[1], PROBE)
        same3([v[1, at2] for v in g2[:3]], [v[1] for v in probe_alone], 'slab 1 probe levels')


# ------------------------------------------------------------------------------------------------------------------- (d) blocks per slab
@pytest.mark.parametrize('rule,S,ny,nx,N,ncopy,bps', [
    ('share', 256, 258, 40, 40, 8, 8),          # ntile 9 > share 8; need 1
    ('floor', 300, 258, 40, 40, 8, 8),          # share 6 -> 8 < ntile 9
    ('capacity', 256, 961, 2, 300, 1, 30),      # one copy: a block may walk ONE tile: need 30 = ntile
    ('capacity', 256, 961, 2, 150, 2, 10),      # two copies: three tiles per block
    ('ntile', 1, 33, 64, 40, 8, 1),
], ids=['share', 'floor', 'capacity-1copy', 'capacity-2copies', 'ntile'])
def test_blocks_per_slab_rules(ctx, rule, S, ny, nx, N, ncopy, bps):
    """four distinct slabs repeated; then the same four alone -- another bps (but for one copy, where the capacity rule asks for a
    block per tile and no launch has another; there the rule differs) --, the same bits"""
    planes = [field(ny, nx, seed=20 + p, noise=0.3).astype(np.float32) for p in range(4)]
    Fs = [noisy((ny, nx), 30 + p, np.float32 if p % 2 else np.float64).astype(np.float64) for p in range(4)]
    index = [(s * 7) % 4 for s in range(S)]
    q, F = np.stack([planes[p] for p in index]), np.stack([Fs[p] for p in index])
    y, x = coords('hashed', ny, nx, False, salt=3)
    lv = levels_in(q[:4], N, seed=1)
    got = run(ctx, q, F, lv, y, x, want=dict(bps_rule=rule, ncopy=ncopy, bps=bps))
    check(got, ref_stack(planes, Fs, index, lv, y, x), rule)
    if S > 4:
        one = run(ctx, q[:4], F[:4], lv, y, x)
        assert (one[3]['bps'], one[3]['bps_rule']) != (got[3]['bps'], got[3]['bps_rule'])
        assert ncopy == 1 or one[3]['bps'] != got[3]['bps']
        same3(one, [v[:4] for v in got[:3]], rule + ' alone')


# ------------------------------------------------------------------------------------------------------------------- (e) saturation
def test_checkerboard_saturates_the_signed_words(ctx):
    """K10's checkerboard -- every cell a saddle across every level, two segments each -- under K15's capacity rule: 200 levels take
    two LDS copies, a block walks three full tiles (24192 cells), so every copy of a level takes 12096 cells x 2 = 24192 chunks per
    word, all of one sign on a slab whose integrand has one sign: as close to the 32766-chunk budget of a signed word as the launch
    rules allow (two copies: at most 3 tiles = 24192; one copy: 1 tile = 16128).  Slab 0: F = -M (float32, M = 8): each term is
    -M len, the same chunks as the length's, negated, on a window 3 bits up: integral == -M length bit for bit.  Slab S-1: F = M on
    the nodes where q = -1 and -M where q = +1, i.e. F = -M q: with levels c = -1 + 2m/1024 every end point and every F(u) = -M c
    is exact, each term is -M c len: all of one sign per level (c = 0: all +-0)"""
    ny, nx, S, M = 32 * 27 + 1, 253, 256, 8.0                               # ntile 27, need 9 > share 8
    cb = np.where(np.indices((ny, nx)).sum(0) % 2 == 0, 1.0, -1.0).astype(np.float32)
    q = np.zeros((S, ny, nx), dtype=np.float32)
    F = np.zeros((S, ny, nx), dtype=np.float32)
    q[0] = cb; q[S - 1] = -cb
    F[0] = -M; F[S - 1] = M * cb
    lv = -1.0 + 2.0 * np.arange(412, 612) / 1024.0
    integ, length, nseg, g = run(ctx, q, F, lv, np.arange(float(ny)), np.arange(float(nx)), False,
                                 want=dict(ncopy=2, ngroup=1, bps=9, bps_rule='capacity', ntile=27))
    ncell = (ny - 1) * (nx - 1)
    assert (nseg[[0, S - 1]] == 2 * ncell).all() and (nseg[1:S - 1] == 0).all()
    assert np.isnan(length[1:S - 1]).all() and np.isnan(integ[1:S - 1]).all()
    gg = (1.0 - lv) / 2.0
    want = 2 * ncell * np.hypot(gg, gg)
    for s in (0, S - 1):
        assert np.max(np.abs(length[s] - want) / want) <= 1e-12
    same_bits(length[0], length[S - 1], 'the two boards')
    same_bits(integ[0], -M * length[0], 'constant slab')
    scale = M * np.abs(lv) * length[S - 1]
    assert (lv == 0).sum() == 1 and np.all(np.abs(integ[S - 1] - -M * lv * length[S - 1]) <= 1e-12 * scale)
    assert (np.sign(integ[S - 1]) == -np.sign(lv)).all()


# ------------------------------------------------------------------------------------------------------------------- (f) edges
RING_X = [2, 63, 64, 252, 253, 504, 505]


@pytest.mark.parametrize('ncy', EDGE_Y)
def test_tile_wave_and_seam_edges(ctx, ncy):
    """nx - 1 (on the ring: nx) across the wave (63 cells) and tile (252) boundaries, ny - 1 across the row batches (4) and tiles (32),
    on the sphere with coordinates and integrands that differ on every node: a coordinate or an integrand corner read from the wrong
    column or row changes the result.  The ring rows also bit for bit against the plain call on the extended plane"""
    ny = ncy + 1
    for n, (ncx, ring) in enumerate([(c, False) for c in EDGE_X] + [(c, True) for c in RING_X]):
        nx = ncx if ring else ncx + 1
        q = np.stack([field(ny, nx, seed=ncx + ncy, noise=0.4), field(ny, nx, seed=ncx * ncy + 1, noise=0.4)])
        F = noisy(q.shape, ncx + 7 * ncy, np.float32 if n % 2 else np.float64)
        y, x = coords('stretched' if n % 2 else 'descending', ny, nx, True, salt=ncx)
        lv = levels_in(q, 17, seed=ncx)
        P = PERIOD_LL if ring else None
        what = 'cells %dx%d%s' % (ncy, ncx, ' ring' if ring else '')
        got = run(ctx, q, F, lv, y, x, True, P, want=dict(ntile=-(-ncy // 32) * -(-ncx // 252)))
        check(got, LR.stack(q, F.astype(np.float64), lv, y, x, True, P), what)
        if ring:
            qe, xe = PR.extend_plane(q, x, P)
            Fe, _ = PR.extend_plane(F, x, P)
            ext = run(ctx, np.ascontiguousarray(qe), np.ascontiguousarray(Fe), lv, y, xe, True)
            same3(got, ext, what + ' against the extended plane')
            assert got[2].sum() > ctx.contour_line_integrals(q, F, lv, y, x, radius=CR.RADIUS)[2].sum() or nx == 2


@pytest.mark.parametrize('shape,ring', [((1, 40), False), ((30, 1), False), ((1, 1), False), ((1, 40), True)])
def test_planes_without_cells(ctx, shape, ring):
    ny, nx = shape
    rng = np.random.default_rng(0)
    q, F = rng.standard_normal((3, ny, nx)), rng.standard_normal((3, ny, nx))
    integ, length, nseg, _ = run(ctx, q, F, [-0.5, 0.0, 0.5], np.arange(ny) * 1.5, np.arange(nx) * 0.5, False, 25.0 if ring else None,
                                 want=dict(ntile=0, bps=0, bps_rule=None))
    assert np.isnan(integ).all() and np.isnan(length).all() and (nseg == 0).all()


# ------------------------------------------------------------------------------------------------------------------- (g) completeness
INST = [(tq, tf, latlon, ring) for tq in (np.float32, np.float64) for tf in (np.float32, np.float64) for latlon in (False, True)
        for ring in (False, True)]


def inst_key(tq, tf, latlon, ring):
    return ('ring' if ring else 'plain', np.dtype(tq).name.replace('float', 'f'), np.dtype(tf).name.replace('float', 'f'), bool(latlon))


@pytest.mark.parametrize('tq,tf,latlon,ring', INST, ids=['-'.join(map(str, inst_key(*i))) for i in INST])
def test_every_instantiation(ctx, tq, tf, latlon, ring):
    ny, nx = 35, 256
    q = np.stack([field(ny, nx, seed=41, noise=0.3), field(ny, nx, seed=42, noise=0.3)]).astype(tq)
    F = noisy(q.shape, 5, tf)
    y, x = coords('descending' if latlon else 'hashed', ny, nx, latlon, salt=6)
    P = (PERIOD_LL if latlon else float(x[-1] - x[0]) * 1.01) if ring else None
    lv = levels_in(q, 31, seed=2)
    got = run(ctx, q, F, lv, y, x, latlon, P, want=dict(ntile=4, ncopy=8))
    ref = LR.stack(q.astype(np.float64), F.astype(np.float64), lv, y, x, latlon, P)
    check(got, ref, '-'.join(map(str, inst_key(tq, tf, latlon, ring))))
    assert (ref[2] > 0).mean() > 0.75


# kernel -> the rows that reach it
ROWS = {inst_key(*i): 'test_every_instantiation[%s]' % '-'.join(map(str, inst_key(*i))) for i in INST}
ROWS.update({'window': 'every row (k_cline_window)', 'finish': 'every row (k_cline_finish)'})


def parse_symbol(s):
    m = re.search(r'(7k_cline|12k_ring_cline)I([df])([df])Lb([01])EE', s)
    if m:
        t = {'d': 'f64', 'f': 'f32'}
        return ('ring' if 'ring' in m.group(1) else 'plain', t[m.group(2)], t[m.group(3)], m.group(4) == '1')
    for k in ('window', 'finish'):
        if 'k_cline_' + k in s:
            return k
    raise AssertionError('unrecognised K15 kernel symbol %s' % s)


def test_every_instantiation_has_a_row(tmp_path):
    """every k_cline* / k_ring_cline* kernel of the gfx950 code object has a row here, and every row names one that exists.  Reads
    symbol names only; runs no kernel."""
    from xcontour_amd import _native as nat
    tool = '/opt/rocm/llvm/bin'
    lib = str(tmp_path / 'lib.so')
    shutil.copy(nat.LIB_PATH, lib)
    subprocess.run([os.path.join(tool, 'llvm-objdump'), '--offloading', lib], check=True, cwd=str(tmp_path), stdout=subprocess.DEVNULL)
    syms = set()
    for f in sorted(os.listdir(str(tmp_path))):
        if 'gfx950' in f:
            out = subprocess.run([os.path.join(tool, 'llvm-readelf'), '-Ws', str(tmp_path / f)], check=True, stdout=subprocess.PIPE,
                                 universal_newlines=True).stdout
            syms |= set(m for m in re.findall(r'\b(_Z\S*k_(?:ring_)?cline\S*)', out) if '.' not in m)
    keys = set(parse_symbol(s) for s in syms)
    assert len(keys) == len(syms) == 18
    assert keys == set(ROWS), 'kernels without a row: %s; rows without a kernel: %s' % (keys - set(ROWS), set(ROWS) - keys)
    assert {inst_key(*i) for i in INST} == {k for k in ROWS if isinstance(k, tuple)} and len(INST) == 16
