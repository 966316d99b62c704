"""Independent numpy statement of the sampled dense-dense product of a tiling (include/pem_spgemm.h pem_tiled_sddmm /
pem_tiled_set_values_sddmm): for every stored position e = (i_e, j_e) of the pattern

    R_e = the left fold over c = 0 .. k-1 of X[i_e, c] (x) Y[j_e, c]

from the semiring's start value -- or from the entry's old value with accumulate (lor_land: from old != 0):
    plus_times  acc = fma(X, Y, acc)              start 0
    min_plus    acc = fmin(acc, X + Y)            start +inf
    max_plus    acc = fmax(acc, X + Y)            start -inf
    max_times   acc = fmax(acc, X * Y)            start -inf
    plus_pair   acc = acc + 1 (X, Y never read)   start 0
    lor_land    acc = 1 if X != 0 and Y != 0 else acc   start 0
Each step is rounded once in the value type.  numpy cannot round an fma once, so plus_times goes through the oracle -- without
forming the dense rows x cols product: entry e gets a row of its own.  A'' is nnz x nnz*k with row e holding X[i_e, :] at columns
e*k .. e*k+k-1, x'' stacks Y[j_e, :]; mxvref's _plus_times of that pair (the oracle product A'' * x'', every element stored, zeros
included, so no chain skips a term) returns every chain in ascending c at O(nnz * k) cost, and brings the [y | A] * [1 ; x] start
for accumulate with its -0.0 patch.  The oracle indexes with int32, so nnz * k must stay below 2^31.

The pattern is (I, J), one pair per entry in any order; the result is in that order.  X and Y are 2-D arrays (any strides).
"""
import numpy as np

import mxvref as mr

SEMIRINGS = mr.SEMIRINGS
START = mr.MXV_START


def sddmm(I, J, X, Y, semiring, dtype, old=None, oracle=None):
    """R_e for every entry (I[e], J[e]); old: the entries' old values (accumulate) or None.  Returns nnz values of dtype."""
    dtype = np.dtype(dtype).type
    I, J = np.asarray(I, np.int64), np.asarray(J, np.int64)
    X, Y = np.asarray(X, dtype), np.asarray(Y, dtype)
    nnz, k = len(I), X.shape[1]
    assert Y.shape[1] == k
    if old is not None:
        old = np.asarray(old, dtype)
    if semiring == "plus_times":
        if nnz == 0:
            return np.zeros(0, dtype)
        if k == 0:
            return np.zeros(nnz, dtype) if old is None else old.copy()
        if oracle is None:
            raise ValueError("plus_times needs the oracle (the fma chain)")
        assert nnz * k < 2 ** 31 - 1
        rp = np.arange(nnz + 1, dtype=np.int64) * k
        ci = np.arange(nnz * k, dtype=np.int64)
        return mr._plus_times(oracle, nnz, nnz * k, rp, ci, np.ascontiguousarray(X[I]).ravel(), np.ascontiguousarray(Y[J]).ravel(), dtype, old)
    if old is None:
        acc = np.full(nnz, START[semiring], dtype)
    else:
        acc = (old != 0).astype(dtype) if semiring == "lor_land" else old.copy()
    one = dtype(1)
    with np.errstate(all="ignore"):
        for c in range(k):
            if semiring == "plus_pair":
                acc = acc + one
                continue
            x, y = X[I, c], Y[J, c]
            if semiring == "lor_land":
                acc = np.where((x != 0) & (y != 0), one, acc)
            elif semiring == "min_plus":
                acc = np.fmin(acc, x + y)
            elif semiring == "max_plus":
                acc = np.fmax(acc, x + y)
            elif semiring == "max_times":
                acc = np.fmax(acc, x * y)
            else:
                raise ValueError(semiring)
    return acc.astype(dtype)


def pattern_of(rows, rp, ci):
    """(I, J) of a CSR pattern, in CSR order"""
    rp = np.asarray(rp, np.int64)
    return np.repeat(np.arange(rows, dtype=np.int64), np.diff(rp)), np.asarray(ci, np.int64)
