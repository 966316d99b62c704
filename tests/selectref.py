"""numpy restatement of select (csrc/select.hip, pem_tiled_select).

The input is a COO triple (I, J, V) of the matrix a tiling represents; the result is the sub-triple of the entries that satisfy the op
with the thunk, in the input's order, values unchanged.  Positional ops compare (i, j) with the integer k = thunk; value ops compare
the value, in `dtype`, with y = thunk rounded once to `dtype` (IEEE comparisons: -0.0 == 0.0, NaN compares false but for !=)."""
import numpy as np

OPS = ("tril", "triu", "diag", "offdiag", "row_le", "row_gt", "col_le", "col_gt", "value_eq", "value_ne", "value_lt", "value_le",
       "value_gt", "value_ge", "abs_gt")
POSITIONAL = OPS[:8]


def positional_thunk_ok(thunk):
    """the rule of pem_tiled_select: an integral k with |k| <= 2^31"""
    t = float(thunk)
    return bool(np.isfinite(t)) and t == np.floor(t) and abs(t) <= 2.0 ** 31


def keep(op, I, J, V, thunk, dtype=np.float64):
    """bool mask of the kept entries"""
    if op not in OPS:
        raise ValueError(op)
    if op in POSITIONAL:
        if not positional_thunk_ok(thunk):
            raise ValueError(f"positional op {op}: thunk {thunk!r} is not an integer k with |k| <= 2^31")
        k = int(thunk)
        i, j = np.asarray(I, np.int64), np.asarray(J, np.int64)
        return dict(tril=j <= i + k, triu=j >= i + k, diag=j == i + k, offdiag=j != i + k, row_le=i <= k, row_gt=i > k, col_le=j <= k,
                    col_gt=j > k)[op]
    dt = np.dtype(dtype)
    x = np.asarray(V, dt)
    y = dt.type(thunk)
    with np.errstate(invalid="ignore"):
        if op == "value_eq":
            return x == y
        if op == "value_ne":
            return x != y
        if op == "value_lt":
            return x < y
        if op == "value_le":
            return x <= y
        if op == "value_gt":
            return x > y
        if op == "value_ge":
            return x >= y
        return np.abs(x) > y


def select(I, J, V, op, thunk=0, dtype=np.float64):
    """the kept (I, J, V), values in dtype"""
    m = keep(op, I, J, V, thunk, dtype)
    return np.asarray(I, np.int32)[m], np.asarray(J, np.int32)[m], np.asarray(V, np.dtype(dtype))[m]
