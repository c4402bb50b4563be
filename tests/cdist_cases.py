"""The inputs of the K27 tests, shared by test_cdist_host.py (which shows on the CPU that cdist_ref tells a wrong rule on exactly these)
and the GPU tests -- a helper, no tests here.  A record case is a dict: rec = (count, e_from, e_to, pts), ny, nx, periodic, period,
ycoord, xcoord, radius."""
import functools

import numpy as np

import cdist_ref as DR
import contour_join_periodic_ref as JP
import contour_join_ref as JR


def smooth(ny, nx, seed, modes=4, periodic=False):
    """a smooth random field: a few Fourier modes (whole waves along x when periodic), so a level has hundreds of segments, not
    one per cell"""
    rng = np.random.default_rng(seed)
    r, c = np.meshgrid(np.arange(ny) / max(ny - 1, 1), np.arange(nx) / (nx if periodic else max(nx - 1, 1)), indexing='ij')
    q = np.zeros((ny, nx))
    for _ in range(modes):
        ky, kx = rng.uniform(0.5, 3.0), (rng.integers(1, 4) if periodic else rng.uniform(0.5, 3.0))
        q += rng.normal() * np.sin(2 * np.pi * (ky * r + rng.random())) * np.cos(2 * np.pi * (kx * c + rng.random()))
    return q


def noise(ny, nx, seed):
    return np.random.default_rng(seed).normal(size=(ny, nx))


def coords(ny, nx, seed, periodic=False, descending=False):
    """non-uniform coordinates -> (ycoord, xcoord, period): ascending, or with `descending` the same values from the top down in both
    directions and, on a ring, a negative period (column nx lies one period BELOW xcoord[0])"""
    rng = np.random.default_rng(seed)
    y = np.cumsum(rng.uniform(0.5, 1.5, ny)) - 3.0
    x = np.cumsum(rng.uniform(0.5, 1.5, nx)) + 10.0
    period = float(x[-1] - x[0] + 1.25) if periodic else 0.0
    if descending:
        return y[::-1].copy(), x[::-1].copy(), -period
    return y, x, period


def case(q, levels, periodic=False, seed=0, radius=0.0, ycoord=None, xcoord=None, period=None, descending=False):
    """one plane and its levels -> the record case of Context.contour_segments' records; ycoord, xcoord and period replace the
    coordinates the case would make"""
    q = np.asarray(q, dtype=np.float64)
    ny, nx = q.shape
    rec = (JP if periodic else JR).stack_records(q[None], np.asarray(levels, dtype=np.float64))
    if radius > 0.0:                                         # a sphere: latitudes short of the poles, longitudes round the ring
        y = np.deg2rad(np.linspace(-80.0, 85.0, ny)); x = DR.RING * np.arange(nx) / nx; p = DR.RING if periodic else 0.0
    else:
        y, x, p = coords(ny, nx, seed + 100, periodic, descending)
    y = y if ycoord is None else np.asarray(ycoord, dtype=np.float64)
    x = x if xcoord is None else np.asarray(xcoord, dtype=np.float64)
    p = p if period is None or not periodic else float(period)
    return dict(rec=rec, ny=ny, nx=nx, periodic=int(periodic), period=p, ycoord=y, xcoord=x, radius=radius)


@functools.lru_cache(maxsize=None)
def ring_field(ny=37, nx=40):
    """level 0 of this field on the ring of columns: a wavy circumpolar ring (the main one), a straight one with fewer segments, and a
    closed blob between them"""
    r, c = np.meshgrid(np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing='ij')
    q = np.minimum(r - 10.3 + 2.0 * np.sin(2 * np.pi * c / nx), 25.5 - r)
    return q - 8.0 * np.exp(-((r - 17.7) ** 2 + (c - 20.2) ** 2) / 3.0)


@functools.lru_cache(maxsize=None)
def ring_case():
    return case(ring_field(), [0.0, 2.0], periodic=True, seed=3)


@functools.lru_cache(maxsize=None)
def plane_cases():
    """name -> case: the plane sizes around a tile (16 x 16: exactly one; 17 x 33: one row and column past it; 37 x 45; two rows), a
    range without segments, smooth levels (one LDS chunk per block) and white noise (more than one)"""
    out = {}
    for name, (ny, nx) in (('16x16', (16, 16)), ('17x33', (17, 33)), ('37x45', (37, 45)), ('2x40', (2, 40))):
        out[name] = case(smooth(ny, nx, ny * nx), [-0.4, 0.1, 99.0], seed=ny)
    out['37x45 noise'] = case(noise(37, 45, 7), [0.0, 0.3], seed=5)
    out['37x40 ring noise'] = case(noise(37, 40, 8), [0.1], periodic=True, seed=6)
    return out


@functools.lru_cache(maxsize=None)
def diamond_case():
    """hand-built records on the integer grid of a 17 x 33 plane (coordinates = indices, every operation exact): the ring
    (4, 8) -> (8, 12) -> (12, 8) -> (8, 4) -> back, and an open two-segment piece with a coincident-end segment.  The centre (8, 8)
    is sqrt(8) from all four sides: the smallest id wins."""
    ny, nx = 17, 33
    v = [(4.0, 8.0), (8.0, 12.0), (12.0, 8.0), (8.0, 4.0)]
    ids = [2 * (4 * nx + 8), 2 * (8 * nx + 11) + 1, 2 * (11 * nx + 8), 2 * (8 * nx + 4) + 1]
    ef = ids + [2 * (14 * nx + 20), 2 * (14 * nx + 24)]
    et = ids[1:] + ids[:1] + [2 * (14 * nx + 24), 2 * (14 * nx + 28)]
    pts = [v[k] + v[(k + 1) % 4] for k in range(4)] + [(14.0, 20.0, 14.0, 24.0), (14.0, 24.0, 14.0, 24.0)]
    rec = (np.array([[6]], dtype=np.uint64), np.array(ef, dtype=np.int64), np.array(et, dtype=np.int64), np.array(pts, dtype=np.float64))
    return dict(rec=rec, ny=ny, nx=nx, periodic=0, period=0.0, ycoord=np.arange(ny, dtype=np.float64), xcoord=np.arange(nx, dtype=np.float64),
                radius=0.0)


def reference(c, select=0, **kw):
    return DR.distance(*c['rec'], c['ny'], c['nx'], c['periodic'], select, c['ycoord'], c['xcoord'], c['period'], c['radius'], **kw)


def shuffled(c, seed=11):
    """the same records, shuffled inside their ranges"""
    cnt, ef, et, pts = c['rec']
    rng, o, s0 = np.random.default_rng(seed), [], 0
    for n in cnt.ravel().astype(np.int64):
        o.append(s0 + rng.permutation(n)); s0 += n
    o = np.concatenate(o) if o else np.empty(0, dtype=np.int64)
    return dict(c, rec=(cnt, ef[o], et[o], pts[o]))


# ------------------------------------------------------------------ planes of more than 256 blocks, ties across blocks, the sphere
def blocks_of(c, r=0):
    """the block index (cdist_ref.BLOCK x BLOCK cells, row-major) of every record of range r"""
    cnt = c['rec'][0].ravel().astype(np.int64)
    s0 = int(cnt[:r].sum())
    node = np.asarray(c['rec'][1][s0:s0 + int(cnt[r])], dtype=np.int64) >> 1
    return (node // c['nx'] // DR.BLOCK) * ((c['nx'] + DR.BLOCK - 1) // DR.BLOCK) + (node % c['nx']) // DR.BLOCK


def nblocks(c):
    return ((c['ny'] + DR.BLOCK - 1) // DR.BLOCK) * ((c['nx'] + DR.BLOCK - 1) // DR.BLOCK)


def straddles_the_scan_chunk(c, r):
    """range r has non-empty blocks below index 256 and at or above it, and an empty block between two non-empty ones"""
    b = np.unique(blocks_of(c, r))
    return bool(b.size and b.min() < 256 <= b.max() and (np.diff(b) > 1).any())


@functools.lru_cache(maxsize=None)
def wide_case():
    """2 x 8225, not periodic: 1 x 258 blocks, more than the 256 the block scan takes at a time.  A smooth field plus a short wave
    along x: the level crosses it in blocks on both sides of block 256, with empty blocks in between.  The empty range comes FIRST."""
    ny, nx = 2, 8225
    q = smooth(ny, nx, 3) + 0.3 * smooth(ny, nx, 4) + 0.8 * np.sin(2 * np.pi * 64 * np.arange(nx) / nx)[None, :]
    c = case(q, [99.0, 0.1, -0.3], seed=2)
    assert nblocks(c) == 258 and int(c['rec'][0].ravel()[0]) == 0
    assert straddles_the_scan_chunk(c, 1) and straddles_the_scan_chunk(c, 2)
    return c


@functools.lru_cache(maxsize=None)
def wide_ring_case():
    """34 x 4130 on the ring of columns: 2 x 130 = 260 blocks, so block 256 lies inside the second block row (node rows 32 and 33).
    Whole waves along x whose phase drifts with the row keep the level crossing those two rows in some blocks and not in others.
    Two ranges: in one group their block tables lie 260 entries apart."""
    ny, nx = 34, 4130
    r, c = np.meshgrid(np.arange(ny) / (ny - 1), np.arange(nx) / nx, indexing='ij')
    q = 0.2 * smooth(ny, nx, 9, periodic=True) + 0.8 * np.sin(2 * np.pi * (16 * c + 0.15 * r)) + 0.5 * (r - 0.5)
    out = case(q, [0.1, -0.4], periodic=True, seed=4)
    assert nblocks(out) == 260
    assert straddles_the_scan_chunk(out, 0) and straddles_the_scan_chunk(out, 1)
    return out


def wide_ring_nodes():
    """the nodes the 34 x 4130 ring is compared on against the brute force: the first and last row and column of every tile row and
    tile column that touches block 255 or 256 (cells of rows 32.., columns 4000 .. 4063), and every 7th node elsewhere"""
    ny, nx = 34, 4130
    rows = set(range(0, ny, 7)) | {32, 33}
    cols = set(range(0, nx, 7))
    for tc in range(4000 // DR.TILE, 4064 // DR.TILE + 1):
        cols |= {tc * DR.TILE, tc * DR.TILE + DR.TILE - 1}
    return np.array(sorted(rows)), np.array(sorted(cols))


def sparse_530_nodes():
    """every 5th row and column of the 70 x 530 ring and its last ones: what the host tests look at, where the whole plane is dear"""
    return np.unique(np.r_[np.arange(0, 70, 5), 69]), np.unique(np.r_[np.arange(0, 530, 5), 529])


@functools.lru_cache(maxsize=None)
def cross_block_tie_case():
    """hand-built records on the integer grid of a 22 x 64 plane (coordinates = indices, every operation exact): two point segments,
    P0 at (20, 16) in block 0 and P1 at (0, 56) in block 1, both open pieces.  For the tile of rows 0 .. 15 and columns 16 .. 31 the
    farthest node from P0 is (0, 31), d2 = 400 + 225 = 625: that is the tile's bound after block 0 (and before it).  The gap from the
    tile to P1 is 56 - 31 = 25: block 1's lower bound is 625 as well, and node (0, 31) is 25 from both points.  P1 has the smaller id
    and sits in the block visited later: only a strict skip rule finds it."""
    ny, nx = 22, 64
    p0, p1 = 2 * (20 * nx + 16), 2 * (0 * nx + 56)
    rec = (np.array([[2]], dtype=np.uint64), np.array([p0, p1], dtype=np.int64), np.array([p0 + 1, p1 + 1], dtype=np.int64),
           np.array([(20.0, 16.0, 20.0, 16.0), (0.0, 56.0, 0.0, 56.0)], dtype=np.float64))
    return dict(rec=rec, ny=ny, nx=nx, periodic=0, period=0.0, ycoord=np.arange(ny, dtype=np.float64), xcoord=np.arange(nx, dtype=np.float64),
                radius=0.0)


def swapped(c):
    """the same records in reversed order (one range)"""
    cnt, ef, et, pts = c['rec']
    return dict(c, rec=(cnt, ef[::-1].copy(), et[::-1].copy(), pts[::-1].copy()))


def ring_with_gradient(ny, nx, seed):
    """a periodic smooth field plus a gradient across the rows: circumpolar rings exist"""
    return smooth(ny, nx, seed, periodic=True) + 1.5 * (np.arange(ny)[:, None] / (ny - 1) - 0.5)


R_EARTH = 6371.2e3


@functools.lru_cache(maxsize=None)
def sphere_cases():
    """name -> case on the sphere, 70 x 100 (3 x 4 blocks, 5 x 7 tiles): latitudes DESCEND from +90 to -90 degrees, both poles exactly;
    longitudes round the ring ascending with period +RING, or descending with period -RING"""
    ny, nx = 70, 100
    q = ring_with_gradient(ny, nx, 10)
    lat = np.deg2rad(np.linspace(90.0, -90.0, ny))
    up = DR.RING * np.arange(nx) / nx
    return {'70x100 lat down': case(q, [-0.3, 0.2], periodic=True, radius=R_EARTH, ycoord=lat, xcoord=up, period=DR.RING),
            '70x100 lat down lon down': case(q, [-0.3, 0.2], periodic=True, radius=R_EARTH, ycoord=lat, xcoord=DR.RING - up, period=-DR.RING)}


EMPTY_AROUND = [99.0, -0.4, 99.0, 0.1, 99.0]             # ranges without segments before, between and after the others


@functools.lru_cache(maxsize=None)
def geometry_cases():
    """name -> case: the record cases of test_gpu_cdist_geometry.py on the plane"""
    out = {'2x8225': wide_case(), '34x4130 ring': wide_ring_case(), 'cross-block tie': cross_block_tie_case()}
    out['37x45 empty around'] = case(smooth(37, 45, 37 * 45), EMPTY_AROUND, seed=37)
    out['70x530 ring'] = case(ring_with_gradient(70, 530, 21 + 530), EMPTY_AROUND, periodic=True, seed=7)
    out['37x45 down'] = case(smooth(37, 45, 37 * 45), [-0.4, 0.1], seed=37, descending=True)
    out['37x40 ring down'] = case(ring_field(), [0.0, 2.0], periodic=True, seed=3, descending=True)
    return out


#: the plane cases on which the model (cdist_ref.pruned) skips blocks -- test_cdist_host.py shows it --, so the kernel must too
PRUNED_FOR_SURE = ('2x8225', '34x4130 ring', '70x530 ring')


def any_case(name):
    for cases in (geometry_cases, plane_cases, sphere_cases):
        if name in cases():
            return cases()[name]
    return {'ring': ring_case, 'diamond': diamond_case}[name]()


@functools.lru_cache(maxsize=None)
def cached_reference(name, select=0, max_dist=0.0, nodes=None, mask_seed=None):
    """reference() of a named case, computed once per process (read-only: the tests share it); nodes: None or the name of a
    function here that gives (rows, cols); mask_seed: a negate_mask of random bits, random_mask(case, mask_seed).  The search over
    the segments is made once per (name, select, nodes): the cap and the mask, which cdist_ref applies after it, reuse its winners."""
    c = any_case(name)
    kw = dict(nodes=None if nodes is None else globals()[nodes]())
    if max_dist or mask_seed is not None:
        kw.update(max_dist=max_dist, negate_mask=None if mask_seed is None else random_mask(c, mask_seed),
                  winners=cached_reference(name, select, 0.0, nodes))
    out = reference(c, select, **kw)
    for v in out.values():
        v.setflags(write=False)
    return out


def random_mask(c, seed):
    """a negate_mask of random bits, one per node of every range"""
    return (np.random.default_rng(seed).random((c['rec'][0].size, c['ny'], c['nx'])) < 0.5).astype(np.uint8)


def nselected(c, select=0):
    """the selected segments of all ranges"""
    return sum(int(idx.size) for idx, _ in DR.selected(*c['rec'], c['ny'], c['nx'], c['periodic'], select))


@functools.lru_cache(maxsize=None)
def model(name, bound='gap'):
    """cdist_ref.pruned on every range of a named plane case, every segment selected -> (per range (d2, edge), the pairs of all
    ranges), computed once per process"""
    c = any_case(name)
    cnt, ef, et, pts = c['rec']
    out, pairs, s0 = [], 0, 0
    for n in cnt.ravel().astype(np.int64):
        sl = slice(s0, s0 + int(n))
        d2, p, edge, _ = DR.pruned(ef[sl], pts[sl], c['ny'], c['nx'], c['ycoord'], c['xcoord'], c['periodic'], c['period'], bound=bound,
                                   nearest=True)
        out.append((d2, edge)); pairs += p; s0 += int(n)
    return out, pairs
