"""The matrices of the triangular-solve tests (test_trsv_cpu.py, test_gpu_trsv.py): small, one per way the schedule or the kernel
can go wrong.  Off-diagonal values are standard normal; every diagonal is +-(the row's abs sum + 1 + U[0, 1)), so every solve stays
finite.  A case is (n, I, J, V) in float64 with the diagonal stored; cases built as a lower triangle serve the upper tests flipped
(i -> n - 1 - i, j -> n - 1 - j), the grid and the random case store both triangles and serve both as they are."""
import numpy as np

DTYPES = (np.float64, np.float32)


def _finish(n, I, J, rng):
    """off-diagonal pattern (I, J) -> values, plus a dominant diagonal"""
    I, J = np.asarray(I, np.int64), np.asarray(J, np.int64)
    assert not np.any(I == J)
    V = rng.standard_normal(len(I))
    s = np.zeros(n)
    np.add.at(s, I, np.abs(V))
    d = (s + 1.0 + rng.random(n)) * rng.choice([-1.0, 1.0], n)
    return n, np.concatenate([I, np.arange(n)]), np.concatenate([J, np.arange(n)]), np.concatenate([V, d])


def flip(case):
    n, I, J, V = case
    return n, n - 1 - I, n - 1 - J, V


def dense_lower(n, seed=1):
    i, j = np.tril_indices(n, -1)
    return _finish(n, i, j, np.random.default_rng(seed + n))


def bidiagonal(n=200):
    i = np.arange(1, n)
    return _finish(n, i, i - 1, np.random.default_rng(2))


def grid_red_black(m=40):
    """the 5-point grid m x m, red points numbered before black ones, both triangles stored"""
    r, c = np.divmod(np.arange(m * m), m)
    red = (r + c) % 2 == 0
    new = np.empty(m * m, np.int64)
    new[np.flatnonzero(red)] = np.arange(int(red.sum()))
    new[np.flatnonzero(~red)] = int(red.sum()) + np.arange(int((~red).sum()))
    I, J = [], []
    for dr, dc in ((0, 1), (1, 0), (0, -1), (-1, 0)):
        ok = (r + dr >= 0) & (r + dr < m) & (c + dc >= 0) & (c + dc < m)
        I.append(new[ok])
        J.append(new[((r + dr) * m + c + dc)[ok]])
    return _finish(m * m, np.concatenate(I), np.concatenate(J), np.random.default_rng(3))


def wide_thin_wide():
    """85 tile rows: 0-39 diagonal only, 40 waits for 0, 41-44 each for the one before, 45-84 each for 44"""
    rng = np.random.default_rng(4)
    I, J = [], []
    for p, q in [(40, 0)] + [(p, p - 1) for p in range(41, 45)] + [(p, 44) for p in range(45, 85)]:
        k = int(rng.integers(1, 6))
        I.append(16 * p + rng.integers(0, 16, k))
        J.append(16 * q + rng.integers(0, 16, k))
    IJ = np.unique(np.stack([np.concatenate(I), np.concatenate(J)]), axis=1)
    return _finish(16 * 85, IJ[0], IJ[1], rng)


def arrow(n=400):
    """a diagonal and a dense last row: one row of n - 1 off-diagonal entries"""
    return _finish(n, np.full(n - 1, n - 1), np.arange(n - 1), np.random.default_rng(5))


def random_full(n=600, density=0.01):
    rng = np.random.default_rng(6)
    m = rng.random((n, n)) < density
    np.fill_diagonal(m, False)
    I, J = np.nonzero(m)
    return _finish(n, I, J, rng)


def cases():
    """name -> (lower case, upper case)"""
    out = {}
    for n in (1, 15, 16, 17, 33):
        c = dense_lower(n)
        out[f"dense_{n}"] = (c, flip(c))
    for name, c in (("bidiagonal_200", bidiagonal()), ("wide_thin_wide", wide_thin_wide()), ("arrow_400", arrow())):
        out[name] = (c, flip(c))
    for name, c in (("grid_40x40_red_black", grid_red_black()), ("random_600", random_full())):
        out[name] = (c, c)
    return out


# the level widths the issue states for the cases, both triangles
WIDTHS = {"dense_1": [1], "dense_15": [1], "dense_16": [1], "dense_17": [1, 1], "dense_33": [1, 1, 1], "bidiagonal_200": [1] * 13,
          "grid_40x40_red_black": [50, 50], "wide_thin_wide": [40, 1, 1, 1, 1, 1, 40], "arrow_400": [24, 1]}


def csr(case, dtype=np.float64, drop=None):
    """(n, rowptr, colidx, vals) with sorted columns; drop: a boolean mask of entries to leave out"""
    n, I, J, V = case
    if drop is not None:
        I, J, V = I[~drop], J[~drop], V[~drop]
    o = np.lexsort((J, I))
    rp = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(I, minlength=n), out=rp[1:])
    return n, rp, J[o], np.asarray(V, dtype)[o]
