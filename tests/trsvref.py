"""Independent numpy statement of the triangular solve on a tiling's triangle (include/pem_spgemm.h pem_tiled_trsv, INTEGRATION.md
section 3x), row by row, and of its level schedule.

T is the chosen triangle of the square matrix as stored; the other side is ignored, and under unit_diag the stored diagonal too.
P = i // 16 (the tile size of the format):
  lower, rows ascending   acc = b_i; the stored a_ij with j < i in ascending j: acc = fma(-a_ij, x_j, acc); x_i = acc / a_ii
  upper, rows descending  acc = b_i; the stored a_ij with j >= 16 (P + 1) in ascending j, then those with i < j < 16 (P + 1) in
                          descending j, the same fma; then the division
(x_i = acc under unit_diag).  The fma is libm's fma / fmaf through ctypes -- numpy cannot round a * x + c once -- and the division
numpy's, one IEEE division in the value type.

Schedule: tile row P waits for tile row Q wherever an entry sits in tile (P, Q) with Q < P (lower) or Q > P (upper);
level(P) = 1 + the largest level it waits for, 1 with none.  A solve is one launch per level wider than merge_width and one per
maximal run of consecutive levels each at most merge_width wide.

Inputs are CSR triples (rowptr, colidx, vals) with sorted columns.

index=: the rows of a larger system that carry an off-diagonal entry, squeezed together (compactref.IndexMap), solve to the same bits
as they do inside it once the tile edge -- the one thing here that depends on where a row sits -- is taken from the original
indices; tests/test_compact_cpu.py holds that equal to the plain solve.
"""
import ctypes
import ctypes.util

import numpy as np

UPLO = ("lower", "upper")
TILE = 16

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fma.restype = ctypes.c_double
_libm.fma.argtypes = (ctypes.c_double,) * 3
_libm.fmaf.restype = ctypes.c_float
_libm.fmaf.argtypes = (ctypes.c_float,) * 3


def fma(a, x, c, dtype=np.float64):
    """a * x + c rounded once in dtype; the arguments hold dtype values"""
    if np.dtype(dtype) == np.float32:
        return np.float32(_libm.fmaf(float(a), float(x), float(c)))
    return np.float64(_libm.fma(float(a), float(x), float(c)))


def trsv(n, rp, ci, v, b, uplo="lower", unit_diag=False, dtype=np.float64, index=None):
    """x = T^-1 b in the order above.  ValueError naming the first row (1-based) without a stored diagonal entry unless unit_diag.
    index: for a system whose rows and columns are a subset of a larger one's, squeezed together in ascending order (compactref.IndexMap),
    the original index of every row -- ascending, n of them.  The tile edge of the upper walk is then the original system's, 16 (index[i]
    // 16 + 1) compared with index[j], so the fmas keep the order they have there; nothing else depends on it."""
    if uplo not in UPLO:
        raise ValueError(f"unknown uplo {uplo!r}")
    dtype = np.dtype(dtype).type
    f = _libm.fmaf if dtype is np.float32 else _libm.fma
    rp = [int(p) for p in np.asarray(rp)]
    ci = [int(j) for j in np.asarray(ci)]
    at = list(range(n)) if index is None else [int(t) for t in np.asarray(index)]
    assert len(at) == n and all(p < q for p, q in zip(at, at[1:])), "index: one ascending original index per row"
    a = [float(t) for t in np.asarray(v, dtype)]
    bb = [float(t) for t in np.asarray(b, dtype)]
    if not unit_diag:
        for i in range(n):
            if i not in ci[rp[i]:rp[i + 1]]:
                raise ValueError(f"row {i + 1} has no stored diagonal entry")
    x = [0.0] * n
    upper = uplo == "upper"
    with np.errstate(all="ignore"):
        for i in (range(n - 1, -1, -1) if upper else range(n)):
            ks = range(rp[i], rp[i + 1])
            if upper:
                edge = TILE * (at[i] // TILE + 1)
                walk = [k for k in ks if at[ci[k]] >= edge] + [k for k in reversed(ks) if i < ci[k] and at[ci[k]] < edge]
            else:
                walk = [k for k in ks if ci[k] < i]
            acc = bb[i]
            for k in walk:
                acc = f(-a[k], x[ci[k]], acc)
            if not unit_diag:
                d = [a[k] for k in ks if ci[k] == i][0]
                acc = float(dtype(acc) / dtype(d))
            x[i] = acc
    return np.array(x, dtype)


def levels(n, rp, ci, uplo="lower", index=None):
    """the level (1-based) of every tile row, as an int array of ceil(n / 16) entries.  index (as in trsv): the tile rows are the
    original system's, index[i] // 16, and the result holds the levels of those among them that hold a row of this system, ascending;
    a tile row of the original system that holds none of these rows waits for nothing there: level 1."""
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    I = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    if index is None:
        tr = (n + TILE - 1) // TILE
        I, J = I // TILE, ci // TILE
    else:
        index = np.asarray(index, np.int64)
        assert len(index) == n and np.all(np.diff(index) > 0), "index: one ascending original index per row"
        lines, at = np.unique(index // TILE, return_inverse=True)
        tr = len(lines)
        I, J = at[I], at[ci]
    deps = [set() for _ in range(tr)]
    for p, q in zip(I.tolist(), J.tolist()):
        if (q > p) if uplo == "upper" else (q < p):
            deps[p].add(q)
    lv = [0] * tr
    for p in (range(tr - 1, -1, -1) if uplo == "upper" else range(tr)):
        lv[p] = 1 + max((lv[q] for q in deps[p]), default=0)
    return np.array(lv, np.int64)


def widths(lv):
    """tile rows per level, level 1 first"""
    lv = np.asarray(lv, np.int64)
    return np.bincount(lv, minlength=2)[1:].tolist() if len(lv) else []


def launches(lv, merge_width):
    """the launches of one solve: a level wider than merge_width is one, a maximal run of narrower levels is one"""
    n, in_run = 0, False
    for w in widths(lv):
        if w > merge_width:
            n, in_run = n + 1, False
        elif not in_run:
            n, in_run = n + 1, True
    return n
