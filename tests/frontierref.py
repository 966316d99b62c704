"""Independent numpy statement of the frontier products and the breadth-first search of a tiling (include/pem_spgemm.h
pem_tiled_mxv_frontier / pem_tiled_bfs).

mxv_frontier is mxvref.mxv on the matrix that keeps only the entries whose x_j is present: the fold of an allowed output runs over
those entries in ascending index from the start value (or from the old y with accumulate, where an output without a term stays as
it is); a disallowed output keeps the old y whatever happens; present_out is 1 where an output is allowed and its filtered row is
not empty.  The absent x positions are zeroed before anything reads x, so no value there can reach the model's result.

line_flags states the mark rule: output line L (16 rows of the oriented matrix) is flagged exactly when it stores a tile whose
16-entry x segment has a present entry.

Inputs are CSR triples (rowptr, colidx, vals) with sorted columns, as in mxvref.
"""
import numpy as np

import mxvref as mr


def _oriented(rows, cols, rp, ci, v, transpose):
    if transpose:
        rp, ci, v = mr.transpose_csr(rows, cols, rp, ci, v)
        rows, cols = cols, rows
    return rows, cols, np.asarray(rp, np.int64), np.asarray(ci, np.int64), np.asarray(v)


def allowed_of(n, mask, complement):
    if mask is None:
        return np.ones(n, bool)
    return (np.asarray(mask) != 0) != bool(complement)


def filter_present(rows, rp, ci, v, present):
    """the CSR keeping only the entries whose column is present"""
    keep = np.asarray(present)[ci] != 0
    I = np.repeat(np.arange(rows, dtype=np.int64), np.diff(rp))[keep]
    frp = np.zeros(rows + 1, np.int64)
    np.cumsum(np.bincount(I, minlength=rows), out=frp[1:])
    return frp, ci[keep], v[keep]


def mxv_frontier(rows, cols, rp, ci, v, x, semiring, dtype, present=None, mask=None, complement=False, y_old=None, accumulate=False,
                 oracle=None, transpose=False):
    """(y, present_out) of the rows x cols CSR matrix (transpose: of its transpose).  x may be None under plus_pair; present / mask:
    byte or bool arrays or None (all present / all allowed); y_old: what y held before the call (None: the start value everywhere)"""
    dtype = np.dtype(dtype).type
    rows, cols, rp, ci, v = _oriented(rows, cols, rp, ci, v, transpose)
    present = np.ones(cols, bool) if present is None else np.asarray(present) != 0
    frp, fci, fv = filter_present(rows, rp, ci, v, present)
    xs = np.zeros(cols, dtype)
    if x is not None:
        xs[present] = np.asarray(x, dtype)[present]
    if y_old is None:
        y_old = np.full(rows, mr.MXV_START[semiring], dtype)
    y_old = np.asarray(y_old, dtype)
    res = mr.mxv(rows, cols, frp, fci, fv, xs, semiring, dtype, y0=y_old if accumulate else None, oracle=oracle)
    allowed = allowed_of(rows, mask, complement)
    return np.where(allowed, res, y_old).astype(dtype), (allowed & (np.diff(frp) > 0)).astype(np.uint8)


def line_flags(rows, cols, rp, ci, present, transpose=False):
    """uint8 per output line: 1 where the line stores a tile whose x segment has a present entry"""
    rows, cols, rp, ci, _ = _oriented(rows, cols, rp, ci, np.zeros(len(ci)), transpose)
    present = np.asarray(present) != 0
    nseg = (cols + 15) // 16
    word_on = np.zeros(nseg, bool)
    np.logical_or.at(word_on, np.arange(cols) // 16, present)
    I = np.repeat(np.arange(rows, dtype=np.int64), np.diff(rp))
    flags = np.zeros((rows + 15) // 16, np.uint8)
    flags[np.unique(I[word_on[ci // 16]] // 16)] = 1
    return flags


def bfs(n, rp, ci, source, transpose=False):
    """(levels int32[n], depth, reached): a stored entry (i, j) is an edge i -> j (transpose: j -> i); -1 where unreachable"""
    _, _, rp, ci, _ = _oriented(n, n, rp, ci, np.zeros(len(ci)), transpose)
    level = np.full(n, -1, np.int32)
    level[source] = 0
    frontier = np.array([source], np.int64)
    depth = 0
    while len(frontier):
        nxt = np.unique(np.concatenate([ci[rp[u]:rp[u + 1]] for u in frontier] + [np.zeros(0, np.int64)]))
        nxt = nxt[level[nxt] < 0]
        if not len(nxt):
            break
        depth += 1
        level[nxt] = depth
        frontier = nxt
    return level, depth, int((level >= 0).sum())
