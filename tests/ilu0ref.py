"""Independent numpy statement of ILU(0) on a tiling's own pattern (include/pem_spgemm.h pem_tiled_ilu0),
entry by entry.

A is square with stored pattern S.  F has exactly S and stores L's strict lower triangle (unit diagonal, not stored) and U with its
diagonal.  With m = min(i, j), for every stored (i, j):

    acc = a_ij
    for k ascending over { k < m : (i, k) in S and (k, j) in S }:  acc = fma(-f_ik, f_kj, acc)
    f_ij = acc / f_jj   if j < i   (one IEEE division in the value type)
    f_ij = acc          otherwise

A position that is not stored is never multiplied.  The fma is libm's fma / fmaf through ctypes, as in trsvref, and the division
numpy's.  Inputs are CSR triples (rowptr, colidx, vals) with sorted columns; the result is in the same order.
"""
import numpy as np

from trsvref import _libm


def ilu0(n, rp, ci, v, dtype=np.float64):
    """(f, longest chain): F's values in the order of v, and the largest number of fmas any entry took.  ValueError naming the
    first row (1-based) without a stored diagonal entry."""
    dtype = np.dtype(dtype).type
    fm = _libm.fmaf if dtype is np.float32 else _libm.fma
    rp = [int(p) for p in np.asarray(rp)]
    ci = [int(j) for j in np.asarray(ci)]
    f = [float(t) for t in np.asarray(v, dtype)]
    where = [dict((ci[e], e) for e in range(rp[i], rp[i + 1])) for i in range(n)]
    for i in range(n):
        if i not in where[i]:
            raise ValueError(f"row {i + 1} has no stored diagonal entry")
    longest = 0
    with np.errstate(all="ignore"):
        for i in range(n):
            row = range(rp[i], rp[i + 1])
            for e in row:
                j = ci[e]
                m = min(i, j)
                acc, chain = f[e], 0
                for ek in row:   # (columns ascend inside a row: k ascends)
                    k = ci[ek]
                    if k >= m:
                        break
                    ekj = where[k].get(j)
                    if ekj is not None:
                        acc = fm(-f[ek], f[ekj], acc)
                        chain += 1
                if j < i:
                    acc = float(dtype(acc) / dtype(f[where[j][j]]))
                f[e] = acc
                longest = max(longest, chain)
    return np.array(f, dtype), longest


def pivots(n, rp, ci, f):
    """(zero_pivots, first_zero_pivot_row) as pem_tiled_ilu0_info counts them: the rows whose f_ii is +-0, not finite or not stored,
    and the first of them 1-based (0 if none)"""
    rp, ci, f = np.asarray(rp, np.int64), np.asarray(ci, np.int64), np.asarray(f)
    I = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    d = I == ci
    good = np.zeros(n, bool)
    good[I[d]] = (f[d] != 0) & np.isfinite(f[d])
    bad = np.flatnonzero(~good)
    return len(bad), int(bad[0]) + 1 if len(bad) else 0
