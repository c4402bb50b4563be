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


def coords(ny, nx, seed, periodic=False):
    """ascending, non-uniform coordinates -> (ycoord, xcoord, period)"""
    rng = np.random.default_rng(seed)
    y = np.cumsum(rng.uniform(0.5, 1.5, ny)) - 3.0
    x = np.cumsum(rng.uniform(0.5, 1.5, nx)) + 10.0
    return y, x, (float(x[-1] - x[0] + 1.25) if periodic else 0.0)


def case(q, levels, periodic=False, seed=0, radius=0.0):
    """one plane and its levels -> the record case of Context.contour_segments' records"""
    q = np.asarray(q, dtype=np.float64)
    ny, nx = q.shape
    rec = (JP if periodic else JR).stack_records(q[None], np.asarray(levels, dtype=np.float64))
    if radius > 0.0:                                         # a sphere: latitudes short of the poles, longitudes round the ring
        y = np.deg2rad(np.linspace(-80.0, 85.0, ny)); x = DR.RING * np.arange(nx) / nx; period = DR.RING if periodic else 0.0
    else:
        y, x, period = coords(ny, nx, seed + 100, periodic)
    return dict(rec=rec, ny=ny, nx=nx, periodic=int(periodic), period=period, ycoord=y, xcoord=x, radius=radius)


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
