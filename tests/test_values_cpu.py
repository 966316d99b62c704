"""CPU: the index layout of the numeric refresh (pem_tiled_set_values*, values.hip).

The order maps are built on the device by a count, a scan and a write -- no sort.  Here the same construction is restated
in numpy over the oracle's tiled arrays and compared with what the two orders mean: np.lexsort of the entries' (row, col)
resp. (col, row).  This pins the slot layout the kernels use: (tile row, local row, tile) for the row-major order and
(tile column, local column, CSC position) for the column-major one.  And the entry points refuse null handles without a GPU.
"""
import ctypes as C

import numpy as np
import pytest

from matgen import cases

CASES = cases()


def _popc16(x):
    x = x.astype(np.uint32)
    return np.array([bin(v).count("1") for v in range(1 << 16)], np.int32)[x]


def _entries(t):
    """per entry in tile storage order: tile id, local row, local column, global row, global column"""
    tile = np.repeat(np.arange(t.ntiles), np.diff(t.tile_nnz_ptr))
    r = (t.rowcolidx >> 4).astype(np.int64)
    c = (t.rowcolidx & 15).astype(np.int64)
    R = (t.tile_keys[tile] >> 32).astype(np.int64)
    TC = (t.tile_keys[tile] & 0xFFFFFFFF).astype(np.int64)
    return tile, r, c, 16 * R + r, 16 * TC + c


def _exclusive_scan(x):
    return np.concatenate([[0], np.cumsum(x)])[:-1]


def row_major_map(t):
    """vmap_rows_kernel<false> -> exclusive_scan_i32 -> vmap_rows_kernel<true>"""
    T = t.ntiles
    tid = np.repeat(np.arange(T), 16)
    r = np.tile(np.arange(16), T)
    R = (t.tile_keys[tid] >> 32).astype(np.int64)
    b = t.tile_rowptr[R].astype(np.int64)
    n = t.tile_rowptr[R + 1].astype(np.int64) - b
    slot = 16 * b + r * n + (tid - b)
    slots = np.zeros(16 * T, np.int64)
    slots[slot] = _popc16(t.masks)
    scan = _exclusive_scan(slots)
    tile, lr, _, _, _ = _entries(t)
    e = np.arange(t.nnz)
    k = e - (t.tile_nnz_ptr[tile] + t.rowptr[16 * tile + lr])              # rank inside the tile's row
    return scan[slot[16 * tile + lr]] + k


def col_major_map(t):
    """vmap_cols_kernel<false> -> exclusive_scan_i32 -> vmap_cols_kernel<true>"""
    T = t.ntiles
    p = np.repeat(np.arange(T), 16)
    c = np.tile(np.arange(16), T)
    tid = t.tile_offsets[p].astype(np.int64)
    TC = (t.tile_keys[tid] & 0xFFFFFFFF).astype(np.int64)
    b = t.tile_colptr[TC].astype(np.int64)
    m = t.tile_colptr[TC + 1].astype(np.int64) - b
    slots = np.zeros(16 * T, np.int64)
    slot_of = np.zeros(16 * T, np.int64)                                     # indexed by 16 * tile + local column
    slot_of[16 * tid + c] = 16 * b + c * m + (p - b)
    slots[slot_of[16 * tid + c]] = _popc16(t.masks_t[16 * tid + c])
    scan = _exclusive_scan(slots)
    tile, lr, lc, _, _ = _entries(t)
    k = _popc16(t.masks_t[16 * tile + lc] & ((1 << lr) - 1))                # rank inside the tile's column
    return scan[slot_of[16 * tile + lc]] + k


def _inverse(order):
    inv = np.empty(len(order), np.int64)
    inv[order] = np.arange(len(order))
    return inv


_TILED = {}


def _tilings(oracle, name):
    if name not in _TILED:
        rows, cols, I, J, V, tr = CASES[name]
        ts = [oracle.Tiled(rows, cols, I, J, V, False)]
        if tr:
            ts.append(oracle.Tiled(rows, cols, I, J, V, True))
        _TILED.clear()
        _TILED[name] = ts
    return _TILED[name]


@pytest.mark.parametrize("name", list(CASES))
def test_order_maps_are_the_sorted_orders(oracle, name):
    rows, cols, I, J, V, tr = CASES[name]
    for t in _tilings(oracle, name):
        _, _, _, gr, gc = _entries(t)
        want_row = _inverse(np.lexsort((gc, gr)))       # entry -> its position in (row, col) order
        want_col = _inverse(np.lexsort((gr, gc)))       # ... in (col, row) order
        got_row, got_col = row_major_map(t), col_major_map(t)
        assert np.array_equal(got_row, want_row), f"{name}: row-major map"
        assert np.array_equal(got_col, want_col), f"{name}: column-major map"
        assert t.nnz == 0 or (got_row.min() == 0 and got_row.max() == t.nnz - 1)
        # values gathered through the map are the tiling's own vals (a CSR-ordered array refreshes to the same tiling)
        csr_vals = np.empty(t.nnz)
        csr_vals[want_row] = t.vals
        assert np.array_equal(csr_vals[got_row], t.vals)
    if tr:
        # the A^T tiling's column-major order is the source's CSR order: one array serves A ("row") and A^T ("col")
        A, At = _tilings(oracle, name)
        src = np.lexsort((J, I))                        # source entries in CSR order
        csr = np.asarray(V, np.float64)[src]
        assert np.array_equal(csr[row_major_map(A)], A.vals)
        assert np.array_equal(csr[col_major_map(At)], At.vals)


def test_entry_points_refuse_null_handles_without_a_device(pkg):
    lib = pkg.lib()
    v = np.zeros(4)
    f = np.zeros(4, np.float32)
    for fn, arr in ((lib.pem_tiled_set_values, v), (lib.pem_tiled_set_values_device, v), (lib.pem_tiled_set_values_f32, f),
                    (lib.pem_tiled_set_values_device_f32, f)):
        ptr = arr.ctypes.data_as(C.c_void_p)
        assert fn(None, None, ptr, 0) == -1             # PEM_E_INVALID: null context and tiling
        assert fn(C.c_void_p(1), None, ptr, 0) == -1    # null tiling (the context is not looked at first)
        assert fn(None, C.c_void_p(1), ptr, 1) == -1    # null context
    assert pkg.VALUE_ORDERS == {"row": 0, "col": 1}
