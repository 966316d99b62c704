"""numpy restatement of extract and transpose (csrc/extract.hip, pem_tiled_extract / pem_tiled_transpose).

The input is a COO triple (I, J, V) of the rows x cols matrix a tiling represents (no duplicate positions) plus the index lists RI and
CJ (None = all, in order); the result is the canonical COO -- sorted by (row, column) -- of R = A(RI, CJ): R stores (p, q) exactly
where A stores (RI[p], CJ[q]), with that value unchanged.  Lists may be in any order and may repeat indices; explicit zeros stay
entries.  Values are only moved by index, so every bit pattern survives."""
import numpy as np


def check_list(L, dim, name="list"):
    """the rule of pem_tiled_extract for a non-null list: 1 .. INT32_MAX indices, each in 0 .. dim - 1"""
    L = np.asarray(L)
    if L.ndim != 1 or L.size < 1 or L.size > 2 ** 31 - 1:
        raise ValueError(f"{name}: want 1 .. INT32_MAX indices, got shape {L.shape}")
    if L.dtype.kind not in "iu":
        raise ValueError(f"{name}: indices must be integers, not {L.dtype}")
    if int(L.min()) < 0 or int(L.max()) >= dim:
        raise ValueError(f"{name}: an index is outside 0 .. {dim - 1}")
    return L.astype(np.int64)


def _expand(starts, counts):
    """the concatenation of the ranges starts[k] .. starts[k] + counts[k] - 1, and for every element the k it came from"""
    total = int(counts.sum())
    owner = np.repeat(np.arange(len(counts), dtype=np.int64), counts)
    first = np.cumsum(counts) - counts
    return starts[owner] + (np.arange(total, dtype=np.int64) - first[owner]), owner


def extract(rows, cols, I, J, V, RI=None, CJ=None):
    """(ni, nj, RI', RJ', RV'): the shape and the canonical COO of A(RI, CJ); RI', RJ' int32, RV' in V's dtype"""
    I, J, V = np.asarray(I, np.int64), np.asarray(J, np.int64), np.asarray(V)
    RI = np.arange(rows, dtype=np.int64) if RI is None else check_list(RI, rows, "rows")
    CJ = np.arange(cols, dtype=np.int64) if CJ is None else check_list(CJ, cols, "cols")
    ni, nj = len(RI), len(CJ)
    # row side: A's entries grouped by row, then every output row p takes row RI[p]'s group
    by_row = np.argsort(I, kind="stable")
    row_start = np.searchsorted(I[by_row], np.arange(rows + 1))
    src, p = _expand(row_start[RI], (row_start[RI + 1] - row_start[RI]))
    e = by_row[src]                                   # entry of A behind every (p, *)
    # column side: every entry in column j goes to every q with CJ[q] == j
    by_col = np.argsort(CJ, kind="stable")
    lo = np.searchsorted(CJ[by_col], J[e], "left")
    hi = np.searchsorted(CJ[by_col], J[e], "right")
    pos, k = _expand(lo, hi - lo)
    q = by_col[pos]
    p, e = p[k], e[k]
    o = np.argsort(p * nj + q, kind="stable")
    return ni, nj, p[o].astype(np.int32), q[o].astype(np.int32), V[e[o]]


def transpose(rows, cols, I, J, V):
    """(cols, rows, I', J', V'): the canonical COO of the transposed matrix"""
    I, J, V = np.asarray(I, np.int64), np.asarray(J, np.int64), np.asarray(V)
    o = np.argsort(J * rows + I, kind="stable")
    return cols, rows, J[o].astype(np.int32), I[o].astype(np.int32), V[o]


def selection(n_out, dim, L, left=True):
    """COO of the selection matrix of the device route P*A*Q: left, the n_out x dim matrix with P[p, L[p]] = 1; right, its transpose
    (dim x n_out, Q[L[q], q] = 1)"""
    L = np.asarray(L, np.int32)
    a = np.arange(n_out, dtype=np.int32)
    return (n_out, dim, a, L, np.ones(n_out)) if left else (dim, n_out, L, a, np.ones(n_out))
