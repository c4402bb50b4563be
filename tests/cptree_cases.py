"""The hand-built planes of the K19 tests (test_cptree_host.py on the CPU, test_gpu_cptree_records.py and test_gpu_cptree.py on the GPU) --
a helper, no tests here.  Every plane is traced at level 0.5; each is the smallest at which one mechanism of the parent walk can fail."""
import numpy as np


def chain(n):
    """n x n, n = 4 m + 1: q = max(|r - h|, |c - h|) % 2 -- (n - 1) / 2 nested square rings in one chain, ring k round (2 k + 1)^2 nodes"""
    h = n // 2
    r, c = np.mgrid[0:n, 0:n]
    return (np.maximum(abs(r - h), abs(c - h)) % 2).astype(np.float64)


def stacked_siblings():
    """a block of ones with two zero holes one above the other; the upper hole holds a one-island in the column in which the lower
    hole's topmost crossing lies: the walk from the lower hole must skip the upper hole AND its island"""
    q = np.zeros((16, 9))
    q[1:15, 1:8] = 1.0
    q[3:8, 2:6] = 0.0                                                        # the upper hole
    q[5, 3] = 1.0                                                            # its island
    q[10:13, 3:6] = 0.0                                                      # the lower hole: topmost crossing V(9, 3)
    return q


def two_blobs():
    q = np.zeros((12, 6))
    q[2:4, 2] = 1.0
    q[6:11, 2:4] = 1.0
    return q


def bands():
    """ny 9, nx 8, for a periodic plane: a band of ones (rows 3 to 5) gives two rings that go round; one blob above them, one hole
    between them, one blob below them.  Without flip the upper ring encloses the lower one, with flip the lower the upper."""
    q = np.zeros((9, 8))
    q[3:6] = 1.0
    q[1, 2] = 1.0
    q[4, 4] = 0.0
    q[7, 5] = 1.0
    return q


def seam():
    """ny 9, nx 8: a blob on columns 5 .. 7, 0 .. 2 with a hole on columns 7, 0, 1 and an island in column 0 -- on a periodic plane three
    rings in a chain, the topmost crossings of hole and island in column 0; on a plain plane open pieces"""
    q = np.zeros((9, 8))
    q[1:8, [5, 6, 7, 0, 1, 2]] = 1.0
    q[3:6, [7, 0, 1]] = 0.0
    q[4, 0] = 1.0
    return q


def open_above():
    """free edges: rows >= 2 are ones (an open line from edge to edge) and a hole below it"""
    q = np.zeros((8, 7))
    q[2:] = 1.0
    q[5, 3] = 0.0
    return q


def open_beside_nan(enclosed):
    """a zero node under a NaN node: its contour loses the two cells above it and is an open piece with a crossing on V(4, 5); a hole
    below it in the same column.  `enclosed`: the ones are a block inside zeros, so the hole has a parent BEHIND the open piece"""
    q = np.ones((10, 9))
    if enclosed:
        q = np.zeros((12, 11))
        q[1:11, 1:10] = 1.0
    q[3, 5] = np.nan
    q[4, 5] = 0.0
    q[7, 5] = 0.0
    return q


def checkerboard():
    r, c = np.mgrid[0:5, 0:5]
    return ((r + c) % 2).astype(np.float64)


def one_node():
    q = np.zeros((5, 6))
    q[2, 3] = 1.0
    return q


def long_walk(enclosed):
    """ny 600, nx 4, for a periodic plane (four columns leave no room for a hole on a plain one): a one-node ring in row 596; `enclosed`:
    inside a block on columns 0 to 2 whose only crossing above it lies on V(0, 1)"""
    q = np.zeros((600, 4))
    if enclosed:
        q[1:599, 0:3] = 1.0
        q[596, 1] = 0.0
    else:
        q[596, 1] = 1.0
    return q


def smooth_noise(ny, nx, seed):
    """a few waves plus noise: rings in rings at most levels"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:ny, 0:nx]
    q = np.sin(2 * np.pi * x / nx) * np.cos(3 * np.pi * y / ny) + np.linspace(-1.0, 1.0, ny)[:, None]
    return q + 0.6 * rng.standard_normal((ny, nx))
