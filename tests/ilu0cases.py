"""The matrices of the ILU(0) tests (test_ilu0_cpu.py, test_gpu_ilu0.py): small, one per way the schedule or the kernel can go
wrong.  Every case stores both triangles and has trsvcases' dominant diagonal, so every factor stays finite.  A case is
(n, I, J, V) in float64 with the diagonal stored."""
import numpy as np

from trsvcases import DTYPES, _finish, csr, grid_red_black, wide_thin_wide   # noqa: F401  (csr and DTYPES: for the tests)


def dense(n):
    """full: the tile edges; from three tile rows on, targets (P, R) with R < P, R = P and R > P"""
    i, j = np.nonzero(~np.eye(n, dtype=bool))
    return _finish(n, i, j, np.random.default_rng(100 + n))


def band(n, half, seed):
    i, j = np.indices((n, n))
    keep = (np.abs(i - j) <= half) & (i != j)
    return _finish(n, i[keep], j[keep], np.random.default_rng(seed))


def symmetrised(case, seed):
    """the case's off-diagonal pattern united with its transpose, new values"""
    n, I, J, _ = case
    off = I != J
    IJ = np.unique(np.stack([np.concatenate([I[off], J[off]]), np.concatenate([J[off], I[off]])]), axis=1)
    return _finish(n, IJ[0], IJ[1], np.random.default_rng(seed))


def double_arrow(n=400):
    """a diagonal, a dense last row and a dense last column: a chain of n - 1 into the last entry, and a tile row of n / 16 tiles"""
    k = np.arange(n - 1)
    last = np.full(n - 1, n - 1)
    return _finish(n, np.concatenate([last, k]), np.concatenate([k, last]), np.random.default_rng(105))


def hubs(n=1600):
    """the first and the last row and column hold one entry per tile: two tile rows of n / 16 = 100 tiles, more than a wave has
    lanes, each met by 98 tile rows of three tiles: the kernel's tile-list search takes another path above 64 tiles"""
    k = np.arange(8, n - 16, 16)
    first, last = np.zeros(len(k), np.int64), np.full(len(k), n - 1)
    I = np.concatenate([first, k, last, k, [0, n - 1]])
    J = np.concatenate([k, first, k, last, [n - 1, 0]])
    return _finish(n, I, J, np.random.default_rng(107))


def random_full(n=300, density=0.05):
    rng = np.random.default_rng(106)
    m = rng.random((n, n)) < density
    np.fill_diagonal(m, False)
    I, J = np.nonzero(m)
    return _finish(n, I, J, rng)


def cases():
    out = {f"dense_{n}": dense(n) for n in (1, 15, 16, 17, 33)}
    out["tridiagonal_200"] = band(200, 1, 102)
    out["band_100_20"] = band(100, 20, 103)
    out["grid_40x40_red_black"] = grid_red_black(40)
    out["wide_thin_wide"] = symmetrised(wide_thin_wide(), 104)
    out["double_arrow_400"] = double_arrow()
    out["random_300"] = random_full()
    out["hubs_1600"] = hubs()
    return out


# the level widths of the lower schedule the cases are built for
WIDTHS = {"dense_1": [1], "dense_15": [1], "dense_16": [1], "dense_17": [1, 1], "dense_33": [1, 1, 1], "tridiagonal_200": [1] * 13,
          "grid_40x40_red_black": [50, 50], "wide_thin_wide": [40, 1, 1, 1, 1, 1, 40], "double_arrow_400": [24, 1], "hubs_1600": [1, 98, 1]}
