"""numpy restatement of the build from triplets with duplicates (csrc/build.hip, pem_tiled_build).

The duplicates of one position are folded strictly in input order, ((v0 op v1) op v2) ..., in the value dtype, each step
ewiseref.apply_op (pem_tiled_ewise's both-stored arithmetic); "first" keeps the value that came first, "second" the one that came
last.  The fold goes by rounds -- round k applies the op to every run longer than k -- because np.add.reduce and reduceat add
pairwise, not sequentially.
"""
import numpy as np

import ewiseref

DUP_OPS = ewiseref.OPS + ("first", "second")


def runs(rows, cols, I, J, transpose=False):
    """(order, start, key): the stable order of the triplets by (row, col) of the built matrix, where every run of equal positions
    starts in it (with the closing length appended) and the distinct keys"""
    I, J = np.asarray(I, np.int64), np.asarray(J, np.int64)
    if transpose:
        I, J, rows, cols = J, I, cols, rows
    if len(I) and (I.min() < 0 or I.max() >= rows or J.min() < 0 or J.max() >= cols):
        raise ValueError("index out of range")
    key = I * cols + J
    order = np.argsort(key, kind="stable")
    ks = key[order]
    head = np.ones(len(ks), bool)
    head[1:] = ks[1:] != ks[:-1]
    start = np.flatnonzero(head)
    return order, np.append(start, len(ks)), ks[start]


def fold(rows, cols, I, J, V, dup="plus", transpose=False):
    """the canonical COO (I, J, V) of the matrix pem_tiled_build makes: rows x cols, or its transpose with transpose=True"""
    if dup not in DUP_OPS:
        raise ValueError(f"unknown dup op {dup!r}")
    V = np.asarray(V)
    order, start, key = runs(rows, cols, I, J, transpose)
    ncols = rows if transpose else cols
    oI, oJ = (key // ncols).astype(np.int32), (key % ncols).astype(np.int32)
    Vs = V[order]
    length = np.diff(start)
    first = start[:-1]
    if dup == "second":
        return oI, oJ, Vs[start[1:] - 1]
    acc = Vs[first].copy()
    if dup != "first":
        for k in range(1, int(length.max()) if len(length) else 0):
            sel = np.flatnonzero(length > k)
            acc[sel] = ewiseref.apply_op(dup, acc[sel], Vs[first[sel] + k])
    return oI, oJ, acc


def with_duplicates(I, J, V, rng, lengths):
    """Entries (distinct positions) -> a shuffled triplet list in which entry e appears lengths[e] times.  Its first copy carries
    V[e]; the further ones carry values drawn from V, so whatever special values V holds turn up among the duplicates."""
    I, J, V = np.asarray(I, np.int32), np.asarray(J, np.int32), np.asarray(V)
    lengths = np.asarray(lengths, np.int64)
    assert len(lengths) == len(I) and (len(I) == 0 or lengths.min() >= 1)
    rep = np.repeat(np.arange(len(I)), lengths)
    vals = V[rng.integers(0, len(V), len(rep))] if len(V) else V[:0]
    firsts = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64) if len(I) else np.zeros(0, np.int64)
    vals[firsts] = V
    p = rng.permutation(len(rep))
    return I[rep][p], J[rep][p], vals[p]
