"""Independent numpy statement of the matrix-vector products and reductions of a tiling (include/pem_spgemm.h pem_tiled_mxv /
pem_tiled_reduce).

Every output is a left fold over its row's stored entries in ascending column (for A^T x: its column's entries in ascending row,
i.e. the rows of A^T), from the start value -- or from the old y with accumulate, where empty rows stay as they are:
  mxv   plus_times  acc = fma(a, x, acc)                  start 0
        min_plus    acc = fmin(acc, a + x)                start +inf
        max_plus    acc = fmax(acc, a + x)                start -inf
        max_times   acc = fmax(acc, a * x)                start -inf
        plus_pair   acc = acc + 1 (x and a never read)    start 0
        lor_land    acc = 1 if a != 0 and x != 0 else acc  start 0 (accumulate: y != 0)
  reduce plus acc + a, times acc * a, min fmin, max fmax, lor (acc != 0 or a != 0), land (acc != 0 and a != 0); identities
        0, 1, +inf, -inf, 0, 1 (lor / land with accumulate: start y != 0)
Each step is rounded once in the value type (numpy arithmetic on arrays of that dtype), one step per entry position in the row,
vectorised over rows.  The fma chain is the one thing numpy cannot round once: plus_times is taken from the oracle's product A*X,
which is that chain; with accumulate, row i of A gets the old y_i in front (a new column 0) and x gets a 1 in front, so the chain
starts there (fma(y, 1, 0) = y, except that y = -0.0 becomes +0.0: patched afterwards, see _plus_times).

Inputs are CSR triples (rowptr, colidx, vals) with sorted columns.
"""
import numpy as np

SEMIRINGS = ("plus_times", "min_plus", "max_plus", "max_times", "plus_pair", "lor_land")
OPS = ("plus", "times", "min", "max", "lor", "land")
MXV_START = {"plus_times": 0.0, "min_plus": np.inf, "max_plus": -np.inf, "max_times": -np.inf, "plus_pair": 0.0, "lor_land": 0.0}
IDENTITY = {"plus": 0.0, "times": 1.0, "min": np.inf, "max": -np.inf, "lor": 0.0, "land": 1.0}


def transpose_csr(rows, cols, rp, ci, v):
    """CSR of the cols x rows transpose, columns sorted"""
    rp = np.asarray(rp, np.int64)
    I = np.repeat(np.arange(rows, dtype=np.int64), np.diff(rp))
    J = np.asarray(ci, np.int64)
    o = np.lexsort((I, J))
    trp = np.zeros(cols + 1, np.int64)
    np.cumsum(np.bincount(J, minlength=cols), out=trp[1:])
    return trp, I[o], np.asarray(v)[o]


def _fold(rp, terms, step, acc):
    """acc[i] = step(... step(step(acc[i], terms[rp[i]]), terms[rp[i] + 1]) ...), vectorised over rows (longest rows first, so step k
    touches only the rows longer than k)"""
    rp = np.asarray(rp, np.int64)
    n = np.diff(rp)
    acc = acc.copy()
    order = np.argsort(-n, kind="stable")
    neg = -n[order]
    with np.errstate(all="ignore"):
        for k in range(int(n.max()) if len(n) else 0):
            m = int(np.searchsorted(neg, -k, side="left"))   # the rows longer than k are order[:m]
            live = order[:m]
            acc[live] = step(acc[live], terms[rp[live] + k])
    return acc


def _start(rows, y0, start, dtype, boolean=False):
    if y0 is None:
        return np.full(rows, start, dtype)
    y0 = np.asarray(y0, dtype)
    return (y0 != 0).astype(dtype) if boolean else y0.copy()


def _finish(rp, acc, y0, dtype):
    """accumulate: empty rows keep the old y bit for bit"""
    if y0 is not None:
        empty = np.diff(np.asarray(rp, np.int64)) == 0
        acc[empty] = np.asarray(y0, dtype)[empty]
    return acc


def _plus_times(oracle, rows, cols, rp, ci, v, x, dtype, y0):
    f32 = np.dtype(dtype) == np.float32
    rp = np.asarray(rp, np.int64)
    ci = np.asarray(ci, np.int64)
    I = np.repeat(np.arange(rows, dtype=np.int64), np.diff(rp))
    if y0 is None:   # A * X, X the cols x 1 matrix storing every x_j
        A = oracle.Csr(rows, cols, I, ci, np.asarray(v, np.float64))
        X = oracle.Csr(cols, 1, np.arange(cols), np.zeros(cols, np.int64), np.asarray(x, np.float64))
        crp, _, cv = oracle.csr_spgemm(A, X, f32=f32).arrays()
        out = np.zeros(rows, dtype)
        out[np.diff(crp) > 0] = np.asarray(cv).astype(dtype)
        return out
    # [y | A] * [1 ; x]: every chain starts with fma(y_i, 1, 0) = y_i
    A = oracle.Csr(rows, cols + 1, np.concatenate([np.arange(rows, dtype=np.int64), I]), np.concatenate([np.zeros(rows, np.int64), ci + 1]),
                   np.concatenate([np.asarray(y0, np.float64), np.asarray(v, np.float64)]))
    X = oracle.Csr(cols + 1, 1, np.arange(cols + 1), np.zeros(cols + 1, np.int64), np.concatenate([np.ones(1), np.asarray(x, np.float64)]))
    _, _, cv = oracle.csr_spgemm(A, X, f32=f32).arrays()
    out = np.asarray(cv).astype(dtype)
    # ... except y = -0.0, which that start turns into +0.0: the true chain stays -0.0 while every product is an exact -0.0
    y0 = np.asarray(y0, dtype)
    a, xv = np.asarray(v, dtype), np.asarray(x, dtype)[ci]
    with np.errstate(all="ignore"):
        negzero = (a * xv == 0) & (np.signbit(a) ^ np.signbit(xv)) & np.isfinite(a) & np.isfinite(xv)
    bad = np.concatenate([[0], np.cumsum(~negzero)])
    fix = np.signbit(y0) & (y0 == 0) & (bad[rp[1:]] - bad[rp[:-1]] == 0)
    out[fix] = np.dtype(dtype).type(-0.0)
    return out


def mxv(rows, cols, rp, ci, v, x, semiring, dtype, y0=None, oracle=None, transpose=False):
    """y = A (+).(x) x (transpose: A^T (+).(x) x) of the rows x cols CSR matrix; y0: the old y (accumulate) or None"""
    dtype = np.dtype(dtype).type
    if transpose:
        rp, ci, v = transpose_csr(rows, cols, rp, ci, v)
        rows, cols = cols, rows
    rp = np.asarray(rp, np.int64)
    a = np.asarray(v, dtype)
    xv = np.asarray(x, dtype)[np.asarray(ci, np.int64)]
    if semiring == "plus_times":
        if oracle is None:
            raise ValueError("plus_times needs the oracle (the fma chain)")
        out = _plus_times(oracle, rows, cols, rp, ci, v, np.asarray(x, dtype), dtype, None if y0 is None else np.asarray(y0, dtype))
        if y0 is None:
            return out
        return _finish(rp, out, y0, dtype)
    acc = _start(rows, y0, MXV_START[semiring], dtype, boolean=semiring == "lor_land")
    with np.errstate(all="ignore"):
        if semiring == "plus_pair":
            acc = _fold(rp, np.zeros(len(a), dtype), lambda s, t: s + dtype(1), acc)
        elif semiring == "lor_land":
            hit = ((a != 0) & (xv != 0)).astype(dtype)
            acc = _fold(rp, hit, lambda s, t: np.where(t != 0, dtype(1), s), acc)
        else:
            t = a + xv if semiring in ("min_plus", "max_plus") else a * xv
            acc = _fold(rp, t, np.fmin if semiring == "min_plus" else np.fmax, acc)
    return _finish(rp, acc, y0, dtype)


def reduce(rows, cols, rp, ci, v, op, dtype, y0=None, dim="rows"):
    """the op-fold of every row (dim="cols": every column) of the rows x cols CSR matrix"""
    dtype = np.dtype(dtype).type
    if dim == "cols":
        rp, ci, v = transpose_csr(rows, cols, rp, ci, v)
        rows, cols = cols, rows
    rp = np.asarray(rp, np.int64)
    a = np.asarray(v, dtype)
    one, zero = dtype(1), dtype(0)
    step = {"plus": lambda s, t: s + t, "times": lambda s, t: s * t, "min": np.fmin, "max": np.fmax,
            "lor": lambda s, t: np.where((s != 0) | (t != 0), one, zero), "land": lambda s, t: np.where((s != 0) & (t != 0), one, zero)}[op]
    acc = _start(rows, y0, IDENTITY[op], dtype, boolean=op in ("lor", "land"))
    return _finish(rp, _fold(rp, a, step, acc), y0, dtype)
