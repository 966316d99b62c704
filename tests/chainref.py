"""numpy restatement of the chained-product conversion (csrc/chain.hip): the tile payload of the tiling pem_tiled_from_cplan makes
from a plan's C arrays, untransposed and transposed, and the map its refresh gathers C^T's values through.

C's arrays (include/pem_spgemm.h, pem_cplan_array): c_tile_rowidx (absolute tile row), c_tile_colidx, c_mask (uint32[8 T_C], word q =
(row 2q) << 16 | row 2q+1), c_tile_nnz_ptr, c_vals (row-major inside a tile, tiles in (tile row, tile column) order).
"""
import numpy as np


def row_masks(c_mask):
    """uint16[T_C, 16]: the column mask of every row of every C tile"""
    w = np.asarray(c_mask, np.uint32).reshape(-1, 8)
    out = np.zeros((len(w), 16), np.uint16)
    out[:, 0::2] = (w >> 16).astype(np.uint16)
    out[:, 1::2] = (w & 0xFFFF).astype(np.uint16)
    return out


def _entries(masks):
    """per tile, its (r << 4 | c) bytes in row-major order"""
    return [np.array([(r << 4) | c for r in range(16) for c in range(16) if (int(m[r]) >> c) & 1], np.uint8) for m in masks]


def payload(c, rows, cols, transpose=False):
    """the tile payload (tile_keys, tile_nnz_ptr, rowcolidx, vals) of C's tiling -- or C^T's -- and, for C^T, cmap: the position of
    every entry's value in c_vals"""
    ptr = np.asarray(c["c_tile_nnz_ptr"], np.int64)
    keep = np.flatnonzero(ptr[1:] > ptr[:-1])               # C tiles without entries are dropped
    masks = row_masks(c["c_mask"])[keep]
    tr = np.asarray(c["c_tile_rowidx"], np.int64)[keep]
    tc = np.asarray(c["c_tile_colidx"], np.int64)[keep]
    ents = _entries(masks)
    vals = np.asarray(c["c_vals"])
    if not transpose:
        nnz_ptr = np.concatenate([[0], ptr[keep + 1]]).astype(np.int32)   # (a kept tile starts where the one before it ends)
        return dict(tile_keys=(tr << 32) | tc, tile_nnz_ptr=nnz_ptr,
                    rowcolidx=np.concatenate(ents) if ents else np.zeros(0, np.uint8), vals=vals.copy())
    # C^T: C's tiles in (tile column, tile row) order; inside a tile, C's entries in (c, r) order
    order = np.lexsort((tr, tc))
    keys, rc, cmap, counts = [], [], [], []
    for t in order:
        e = ents[t].astype(np.int64)
        r, cc = e >> 4, e & 15
        o = np.lexsort((r, cc))                              # column-major inside the C tile
        keys.append((tc[t] << 32) | tr[t])
        rc.append(((cc[o] << 4) | r[o]).astype(np.uint8))
        cmap.append(ptr[keep[t]] + o)
        counts.append(len(e))
    cmap = np.concatenate(cmap) if cmap else np.zeros(0, np.int64)
    return dict(tile_keys=np.array(keys, np.int64), tile_nnz_ptr=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32),
                rowcolidx=np.concatenate(rc) if rc else np.zeros(0, np.uint8), vals=vals[cmap], cmap=cmap.astype(np.int32))


def brute_force(I, J, V, transpose=False):
    """the same payload from C's COO entries, sorted by (tile row, tile column, r, c) of the (transposed) matrix"""
    I, J = np.asarray(I, np.int64), np.asarray(J, np.int64)
    if transpose:
        I, J = J, I
    o = np.lexsort((J & 15, I & 15, J >> 4, I >> 4))
    I, J, V = I[o], J[o], np.asarray(V)[o]
    key = ((I >> 4) << 32) | (J >> 4)
    head = np.r_[True, key[1:] != key[:-1]] if len(key) else np.zeros(0, bool)
    starts = np.flatnonzero(head)
    return dict(tile_keys=key[starts], tile_nnz_ptr=np.r_[starts, len(key)].astype(np.int32),
                rowcolidx=(((I & 15) << 4) | (J & 15)).astype(np.uint8), vals=V, order=o)
