"""Independent numpy statement of the arg folds of a tiling (include/pem_spgemm.h pem_tiled_mxv_arg / pem_tiled_reduce_arg /
pem_tiled_bfs_parents), written from the contract: per output, a plain loop over the filtered row.

mxv_arg.  The filtered row of an allowed output keeps the stored entries whose x is present.  Value kinds: every entry's term (a + x
or a * x, one numpy operation in the value type, so rounded once) is a candidate; the winners are the non-NaN terms -- with
accumulate only those strictly better than the old y, unless that is NaN.  With a winner, y is the best winner and idx the smallest
x-index whose term == y; without one, y is the start value and idx -1, or with accumulate both stay as they were.  Index kinds: the
min / max x-index of the filtered row, joined by the old idx where accumulate and idx >= 0; an empty filtered row gives -1 or, with
accumulate, leaves idx alone.  A disallowed output keeps everything.  present_out is 1 where an output is allowed and its filtered
row is not empty.  The absent x positions are never looked at: the terms are computed on the filtered entries only.

Inputs are CSR triples (rowptr, colidx, vals) with sorted columns, as in mxvref / frontierref.
"""
import numpy as np

import mxvref as mr

KINDS = ("min_plus", "max_plus", "max_times", "min_index", "max_index")
VALUE_KINDS = KINDS[:3]
INDEX_KINDS = KINDS[3:]
START = {"min_plus": np.inf, "max_plus": -np.inf, "max_times": -np.inf}


def _oriented(rows, cols, rp, ci, v, transpose):
    if transpose:
        rp, ci, v = mr.transpose_csr(rows, cols, rp, ci, v)
        rows, cols = cols, rows
    return rows, cols, np.asarray(rp, np.int64), np.asarray(ci, np.int64), np.asarray(v)


def _better(kind):
    return (lambda t, y: t < y) if kind == "min_plus" else (lambda t, y: t > y)


def mxv_arg(rows, cols, rp, ci, v, x, kind, dtype, present=None, mask=None, complement=False, y_old=None, idx_old=None, accumulate=False,
            transpose=False):
    """(y, idx, present_out) of the rows x cols CSR matrix (transpose: of its transpose); y is None under an index kind, where x may
    be None.  y_old / idx_old: what y and idx held before the call (None: the start value and -1)"""
    dtype = np.dtype(dtype).type
    rows, cols, rp, ci, v = _oriented(rows, cols, rp, ci, v, transpose)
    values = kind in VALUE_KINDS
    present = np.ones(cols, bool) if present is None else np.asarray(present) != 0
    allowed = np.ones(rows, bool) if mask is None else (np.asarray(mask) != 0) != bool(complement)
    idx = np.full(rows, -1, np.int32) if idx_old is None else np.array(idx_old, np.int32)
    pres = np.zeros(rows, np.uint8)
    y = None
    if values:
        y = np.full(rows, START[kind], dtype) if y_old is None else np.array(y_old, dtype)
        better = _better(kind)
    for i in range(rows):
        if not allowed[i]:
            continue
        js = ci[rp[i]:rp[i + 1]]
        keep = present[js]
        js = js[keep]
        pres[i] = len(js) > 0
        if not values:
            cand = [int(j) for j in js]
            if accumulate and idx[i] >= 0:
                cand.append(int(idx[i]))
            if cand:
                idx[i] = min(cand) if kind == "min_index" else max(cand)
            elif not accumulate:
                idx[i] = -1
            continue
        a = np.asarray(v[rp[i]:rp[i + 1]], dtype)[keep]
        xs = np.asarray(x)[js].astype(dtype)
        with np.errstate(all="ignore"):
            terms = a * xs if kind == "max_times" else a + xs
        old = y[i]
        best = None
        for t in terms.tolist():
            if t != t:
                continue
            if accumulate and old == old and not better(t, float(old)):
                continue   # does not win over the old y
            if best is None or better(t, best):
                best = t
        if best is not None:
            first = next(k for k, t in enumerate(terms.tolist()) if t == best)
            y[i] = terms[first]
            idx[i] = js[first]
        elif not accumulate:
            y[i] = dtype(START[kind])
            idx[i] = -1
    return y, idx, pres


def reduce_arg(rows, cols, rp, ci, v, op, dtype, dim="rows"):
    """(y, idx): per row (dim="cols": column) the min / max stored value and the smallest index where a stored value equals it; the
    identity and -1 for a line that is empty or all NaN"""
    dtype = np.dtype(dtype).type
    rows, cols, rp, ci, v = _oriented(rows, cols, rp, ci, v, dim == "cols")
    y = np.full(rows, mr.IDENTITY[op], dtype)
    idx = np.full(rows, -1, np.int32)
    for i in range(rows):
        vals = np.asarray(v[rp[i]:rp[i + 1]], dtype)
        real = [t for t in vals.tolist() if t == t]
        if not real:
            continue
        best = min(real) if op == "min" else max(real)
        k = vals.tolist().index(best)
        y[i], idx[i] = vals[k], ci[rp[i] + k]
    return y, idx


def bfs_parents(n, rp, ci, source, transpose=False):
    """(levels, parents, depth, reached): a stored entry (i, j) is an edge i -> j (transpose: j -> i); parents[source] = source,
    -1 where unreachable, else the least vertex of the previous level with an edge to the vertex"""
    _, _, rp, ci, _ = _oriented(n, n, rp, ci, np.zeros(len(ci)), transpose)
    level = np.full(n, -1, np.int32)
    parent = np.full(n, -1, np.int32)
    level[source], parent[source] = 0, source
    frontier, depth = [int(source)], 0
    while frontier:
        nxt = []
        for u in sorted(frontier):   # ascending: the first to reach a vertex is its least parent
            for w in ci[rp[u]:rp[u + 1]].tolist():
                if level[w] < 0:
                    level[w], parent[w] = depth + 1, u
                    nxt.append(w)
        if not nxt:
            break
        depth += 1
        frontier = nxt
    return level, parent, depth, int((level >= 0).sum())


def candidate_parents(n, rp, ci, level, transpose=False):
    """per vertex, the number of vertices of the previous level with an edge to it"""
    _, _, rp, ci, _ = _oriented(n, n, rp, ci, np.zeros(len(ci)), transpose)
    count = np.zeros(n, np.int64)
    for u in range(n):
        if level[u] < 0:
            continue
        for w in ci[rp[u]:rp[u + 1]].tolist():
            if level[w] == level[u] + 1:
                count[w] += 1
    return count
