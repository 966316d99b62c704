"""numpy restatement of the Kronecker product of two sparse matrices (csrc/kron.hip, pem_tiled_kron).

With A rowsA x colsA and B rowsB x colsB, the result is rowsA * rowsB by colsA * colsB and stores (i * rowsB + k, j * colsB + l) with
the value op(a_ij, b_kl) wherever A stores (i, j) and B stores (k, l): every pair of stored entries is one entry, zeros included.
Indices are formed by broadcasting in int64, values in the dtype itself with one rounding per entry (ewiseref.apply_op: the dtype's
own *, +, fmin, fmax and the lor / land rule)."""
import numpy as np

from ewiseref import apply_op

BINOPS = ("plus", "times", "min", "max", "lor", "land")


def kron(rowsA, colsA, IA, JA, VA, rowsB, colsB, IB, JB, VB, op="times", dtype=None):
    """canonical (rows, cols, I, J, V) of A (x) B under op; I, J int32, V in the dtype (A's by default)"""
    if op not in BINOPS:
        raise ValueError(f"unknown op {op!r}")
    dt = np.dtype(dtype if dtype is not None else np.asarray(VA).dtype)
    rows, cols = int(rowsA) * int(rowsB), int(colsA) * int(colsB)
    if rows > 2 ** 31 - 1 or cols > 2 ** 31 - 1:
        raise OverflowError(f"the result would be {rows} x {cols}")
    IA, JA, IB, JB = (np.asarray(x, np.int64) for x in (IA, JA, IB, JB))
    P = (IA[:, None] * rowsB + IB[None, :]).ravel()
    Q = (JA[:, None] * colsB + JB[None, :]).ravel()
    a, b = np.broadcast_arrays(np.ascontiguousarray(VA, dt)[:, None], np.ascontiguousarray(VB, dt)[None, :])
    V = apply_op(op, np.ascontiguousarray(a).ravel(), np.ascontiguousarray(b).ravel())
    o = np.lexsort((Q, P))
    return rows, cols, P[o].astype(np.int32), Q[o].astype(np.int32), np.asarray(V, dt)[o]
