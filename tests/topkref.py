"""numpy restatement of select top-k (csrc/topk.hip, pem_tiled_select_topk).

The input is a COO triple (I, J, V) of the matrix a tiling represents; the result keeps, of every line (a row for dim "rows", a column
for "cols"), the first min(k, entries of the line) entries in the line's rank order, in the input's order, values unchanged.  Rank
order: numbers before NaNs; among numbers by x descending ("largest"), x ascending ("smallest") or |x| descending ("abs_largest"),
compared in `dtype` with -0.0 == 0.0; equal entries, and NaNs among themselves, by ascending index inside the line."""
import numpy as np

ORDERS = ("largest", "smallest", "abs_largest")
DIMS = ("rows", "cols")


def rank_key(V, order, dtype=np.float64):
    """(key, nan): entries of a line rank by ascending (nan, key); key is computed in dtype, -0.0 folded onto 0.0, 0 for a NaN"""
    if order not in ORDERS:
        raise ValueError(order)
    x = np.asarray(V, np.dtype(dtype))
    nan = np.isnan(x)
    x = np.where(nan, 0, x) + np.dtype(dtype).type(0)   # (-0.0 + 0.0 = 0.0)
    key = {"largest": -x, "smallest": x, "abs_largest": -np.abs(x)}[order] + np.dtype(dtype).type(0)
    assert key.dtype == np.dtype(dtype)
    return key, nan


def keep(I, J, V, order, dim, k, dtype=np.float64):
    """bool mask of the kept entries"""
    if dim not in DIMS:
        raise ValueError(dim)
    if int(k) != k or k < 0:
        raise ValueError(k)
    I, J = np.asarray(I, np.int64), np.asarray(J, np.int64)
    line, idx = (I, J) if dim == "rows" else (J, I)
    key, nan = rank_key(V, order, dtype)
    o = np.lexsort((idx, key, nan, line))   # by line, then NaN class, then rank key, then index in the line
    sl = line[o]
    start = np.flatnonzero(np.r_[True, sl[1:] != sl[:-1]]) if len(sl) else np.zeros(0, np.int64)
    rank = np.arange(len(sl)) - np.repeat(start, np.diff(np.r_[start, len(sl)]))
    m = np.zeros(len(sl), bool)
    m[o] = rank < k
    return m


def select_topk(I, J, V, order, dim, k, dtype=np.float64):
    """the kept (I, J, V) in input order, values in dtype"""
    m = keep(I, J, V, order, dim, k, dtype)
    return np.asarray(I, np.int32)[m], np.asarray(J, np.int32)[m], np.asarray(V, np.dtype(dtype))[m]
