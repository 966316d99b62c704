"""Independent numpy statement of the sparse-times-dense-block products of a tiling (include/pem_spgemm.h pem_tiled_spmm,
INTEGRATION.md section 3l): column c of Y = A (+).(x) X is mxvref.mxv of column c of X, with the same old column of Y under
accumulate.  X and Y are 2-D row-major arrays and may be column slices of wider arrays (a row stride ld > k); the columns of a wider
Y past k are never touched.
"""
import numpy as np

import mxvref as mr


def spmm(rows, cols, rp, ci, v, X, semiring, dtype, Y0=None, oracle=None, transpose=False):
    """Y = A (+).(x) X (transpose: A^T (+).(x) X) of the rows x cols CSR matrix, X nx x k; Y0: the old Y (accumulate) or None.
    Returns a new ny x k array."""
    X = np.asarray(X, dtype)
    ny = cols if transpose else rows
    k = X.shape[1]
    Y = np.empty((ny, k), dtype)
    for c in range(k):
        y0 = None if Y0 is None else np.ascontiguousarray(np.asarray(Y0, dtype)[:, c])
        Y[:, c] = mr.mxv(rows, cols, rp, ci, v, np.ascontiguousarray(X[:, c]), semiring, dtype, y0=y0, oracle=oracle, transpose=transpose)
    return Y


def spmm_into(rows, cols, rp, ci, v, X, Yfull, k, semiring, dtype, accumulate=False, oracle=None, transpose=False):
    """what the call leaves in a wider row-major buffer Yfull (ny x ldy) whose first k columns are Y: a copy of Yfull with those
    columns replaced, the rest untouched"""
    out = np.array(Yfull, dtype, copy=True)
    out[:, :k] = spmm(rows, cols, rp, ci, v, X, semiring, dtype, Y0=Yfull[:, :k] if accumulate else None, oracle=oracle, transpose=transpose)
    return out
