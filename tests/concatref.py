"""numpy restatement of block assembly (csrc/concat.hip, pem_tiled_concat) on canonical entries.

A grid is a list of lists of blocks, each None (all empty) or (I, J, V) sorted by (row, col) without duplicates; row_sizes[a] and
col_sizes[b] give every cell's shape.  With ro / co the exclusive prefix sums of the sizes, the result is sum(row_sizes) by
sum(col_sizes) and holds (ro_a + i, co_b + j) with the value's bits wherever block (a, b) holds (i, j): shift, concatenate, sort by
(row, col).  gather states the refresh: which (cell, slot) every entry of the result copies."""
import numpy as np


def offsets(sizes):
    s = [int(x) for x in sizes]
    if any(x < 0 for x in s):
        raise ValueError(f"negative size in {s}")
    return np.concatenate([[0], np.cumsum(s, dtype=np.int64)]).astype(np.int64)


def _shifted(blocks, row_sizes, col_sizes):
    """(rows, cols, P, Q, cell, slot) of every entry of every cell, in grid order"""
    ro, co = offsets(row_sizes), offsets(col_sizes)
    if len(blocks) != len(ro) - 1 or any(len(row) != len(co) - 1 for row in blocks):
        raise ValueError("the grid does not match the sizes")
    if ro[-1] > 2 ** 31 - 1 or co[-1] > 2 ** 31 - 1:
        raise OverflowError(f"the result would be {ro[-1]} x {co[-1]}")
    P, Q, cell, slot = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for a, row in enumerate(blocks):
        for b, blk in enumerate(row):
            if blk is None:
                continue
            I, J = np.asarray(blk[0], np.int64), np.asarray(blk[1], np.int64)
            if len(I) and (I.min() < 0 or I.max() >= ro[a + 1] - ro[a] or J.min() < 0 or J.max() >= co[b + 1] - co[b]):
                raise ValueError(f"block ({a}, {b}) does not fit {ro[a + 1] - ro[a]} x {co[b + 1] - co[b]}")
            P.append(I + ro[a])
            Q.append(J + co[b])
            cell.append(np.full(len(I), a * len(row) + b, np.int64))
            slot.append(np.arange(len(I), dtype=np.int64))
    return int(ro[-1]), int(co[-1]), np.concatenate(P), np.concatenate(Q), np.concatenate(cell), np.concatenate(slot)


def gather(blocks, row_sizes, col_sizes):
    """(cell, slot) per entry of the result, in its (row, col) order: entry e is entry slot[e] of the block in cell[e] (row-major)"""
    _, _, P, Q, cell, slot = _shifted(blocks, row_sizes, col_sizes)
    o = np.lexsort((Q, P))
    return cell[o], slot[o]


def concat(blocks, row_sizes, col_sizes, dtype=None):
    """canonical (rows, cols, I, J, V) of the block matrix; I, J int32, V in the dtype (the first block's by default)"""
    some = [blk for row in blocks for blk in row if blk is not None]
    if not some:
        raise ValueError("every block is None")
    dt = np.dtype(dtype if dtype is not None else np.asarray(some[0][2]).dtype)
    rows, cols, P, Q, cell, slot = _shifted(blocks, row_sizes, col_sizes)
    flat = [blk for row in blocks for blk in row]
    V = np.concatenate([np.zeros(0, dt)] + [np.ascontiguousarray(blk[2], dt) for blk in flat if blk is not None])
    o = np.lexsort((Q, P))
    return rows, cols, P[o].astype(np.int32), Q[o].astype(np.int32), V[o]


def refreshed(blocks, row_sizes, col_sizes, values, dtype):
    """the result's values after a refresh: values[k] = the new values of cell k (row-major; None cells ignored)"""
    cell, slot = gather(blocks, row_sizes, col_sizes)
    out = np.zeros(len(cell), np.dtype(dtype))
    for k in np.unique(cell):
        at = cell == k
        out[at] = np.ascontiguousarray(values[int(k)], np.dtype(dtype))[slot[at]]
    return out


def split(I, J, V, row_sizes, col_sizes):
    """the inverse: a list of lists of canonical (I, J, V), piece (a, b) = the entries in its rows and columns, shifted back"""
    ro, co = offsets(row_sizes), offsets(col_sizes)
    I, J, V = np.asarray(I, np.int64), np.asarray(J, np.int64), np.asarray(V)
    out = []
    for a in range(len(ro) - 1):
        out.append([])
        for b in range(len(co) - 1):
            at = (I >= ro[a]) & (I < ro[a + 1]) & (J >= co[b]) & (J < co[b + 1])
            out[-1].append(((I[at] - ro[a]).astype(np.int32), (J[at] - co[b]).astype(np.int32), V[at]))
    return out
