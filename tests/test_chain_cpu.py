"""CPU: chainref (the restatement of csrc/chain.hip) against a brute force that sorts C's COO entries by tile key."""
import numpy as np
import pytest

import chainref


def _plan_arrays(rng, rows, cols, nnz, empty_tiles):
    """C arrays as a plan leaves them: tiles ascending by (tile row, tile column), entries row-major, values in that order, and
    `empty_tiles` listed tiles without entries (PEM_OPT_PRUNE = 0, masked plans)"""
    key = np.unique(rng.choice(rows * cols, size=min(nnz, rows * cols), replace=False))
    I, J = key // cols, key % cols
    o = np.lexsort((J & 15, I & 15, J >> 4, I >> 4))
    I, J = I[o], J[o]
    V = rng.standard_normal(len(I))
    tkey = (I >> 4) * ((cols + 15) // 16) + (J >> 4)
    alltiles = np.arange(((rows + 15) // 16) * ((cols + 15) // 16))
    extra = rng.choice(np.setdiff1d(alltiles, tkey), size=min(empty_tiles, len(np.setdiff1d(alltiles, tkey))), replace=False)
    tiles = np.union1d(np.unique(tkey), extra)
    ntc = len(tiles)
    cnt = np.zeros(ntc, np.int64)
    pos = np.searchsorted(tiles, tkey)
    np.add.at(cnt, pos, 1)
    masks = np.zeros((ntc, 16), np.uint32)
    np.bitwise_or.at(masks, (pos, I & 15), (1 << (J & 15)).astype(np.uint32))
    words = (masks[:, 0::2] << 16) | masks[:, 1::2]
    tc = (cols + 15) // 16
    c = dict(c_tile_rowidx=(tiles // tc).astype(np.int32), c_tile_colidx=(tiles % tc).astype(np.int32), c_mask=words.ravel().astype(np.uint32),
             c_tile_nnz_ptr=np.r_[0, np.cumsum(cnt)].astype(np.int32), c_vals=V)
    return c, I, J, V


SHAPES = [(37, 53, 300, 0), (64, 64, 4096, 0), (200, 90, 900, 25), (16, 16, 256, 0), (33, 300, 40, 60), (40, 40, 0, 7)]


@pytest.mark.parametrize("transpose", (False, True))
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{r}x{c}_{n}_{e}" for r, c, n, e in SHAPES])
def test_payload_matches_brute_force(shape, transpose):
    rows, cols, nnz, empty = shape
    c, I, J, V = _plan_arrays(np.random.default_rng(rows * 7 + nnz), rows, cols, nnz, empty)
    got = chainref.payload(c, rows, cols, transpose)
    want = chainref.brute_force(I, J, V, transpose)
    for k in ("tile_keys", "tile_nnz_ptr", "rowcolidx"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["vals"].view(np.uint64), want["vals"].view(np.uint64))
    if transpose:   # the refresh map: C^T's values gathered from c_vals in C's own order
        assert np.array_equal(got["cmap"], want["order"])
        assert np.array_equal(c["c_vals"][got["cmap"]], got["vals"])
    else:           # untransposed, C's values are the tiling's as they are
        assert np.array_equal(want["order"], np.arange(len(I)))


def test_empty_tiles_are_dropped():
    c, I, J, V = _plan_arrays(np.random.default_rng(3), 200, 90, 50, 40)
    got = chainref.payload(c, 200, 90)
    ptr = got["tile_nnz_ptr"]
    assert len(got["tile_keys"]) < len(c["c_tile_rowidx"])
    assert np.all(np.diff(ptr) >= 1) and np.all(np.diff(ptr) <= 256) and ptr[-1] == len(I)


def test_row_masks_layout():
    # word q holds row 2q in the high half, row 2q+1 in the low half
    m = chainref.row_masks(np.array([(0x1234 << 16) | 0x8001] + [0] * 7, np.uint32))
    assert m[0, 0] == 0x1234 and m[0, 1] == 0x8001 and not m[0, 2:].any()
