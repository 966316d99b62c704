"""GPU: block assembly (pem_tiled_concat), its refresh (pem_tiled_set_values_from_concat), Tiled.split and the CLI's --hstack / --vstack.

The central check is test_gpu_kron.py's: the tiling made on the device equals, array for array, the tiling pem_tiled_from_coo builds
from concatref's entries -- every pem_tiled_info field but the timings, all twelve arrays, values bit for bit.  vals_t is no
pem_tiled_array: it is checked through its readers, mxv(transpose=True) and step 3's B side."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest
import torch

import concatref
from matgen import cases

pytestmark = pytest.mark.gpu

torch.cuda.is_available()   # (torch's runtime first, as in the other GPU files)

CASES = cases()
DTYPES = (np.float64, np.float32)
IDS = ("f64", "f32")
INFO = ("rows", "cols", "nnz", "tile_rows", "tile_cols", "ntiles", "value_bytes")
ARRAYS = ("tile_keys", "tile_nnz_ptr", "masks", "rowptr", "rowcolidx", "vals", "masks_t", "tile_rowptr", "tile_colidx", "tile_colptr",
          "tile_rowidx", "tile_offsets")
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3.0e-310, 1.0e-40, 0.5, -0.5])
UNALIGNED = (1, 14, 1, 1, 14, 33)                                # offsets 0, 1, 15, 16, 17, 31 (and 64 = the end)


def _status(pkg, name):
    return {v: k for k, v in pkg.STATUS_NAMES.items()}[name]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32) if a.dtype.kind == "f" else a


def _same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and bool(np.array_equal(_bits(got), _bits(want)))


def _same_numbers(got, want):
    """results of arithmetic: bit for bit, NaN equals NaN"""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    return bool(np.all((_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want)))) if got.dtype.kind == "f" else bool(np.array_equal(got, want))


def _assert_same_tiling(got, want, label):
    for k in INFO:
        assert getattr(got, k) == getattr(want, k), f"{label}: {k} {getattr(got, k)} != {getattr(want, k)}"
    for name in ARRAYS:
        g, w = got.array(name), want.array(name)
        assert _same_bits(g, w), f"{label}: array {name} differs"


def _specials(rng, v):
    """about a fifth of v replaced by +-0, +-inf, NaN and subnormals"""
    w = np.array(v, np.float64)
    sp = rng.random(len(w)) < 0.2
    w[sp] = rng.choice(SPECIAL, int(sp.sum()))
    return w


def _dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()   # (the vectors are read on the context's stream)
    return t


class Blk:
    """a block: the tiling and the canonical entries of the matrix it represents"""

    def __init__(self, pkg, ctx, rows, cols, I, J, V, dtype, transposed=False):
        V = np.asarray(V, dtype)
        self.T = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, bool(transposed), dtype=dtype)
        if transposed:                                           # a tiling built with transpose = 1 is the tiling of its own matrix
            rows, cols, I, J = cols, rows, J, I
        self.rows, self.cols, self.dtype = rows, cols, dtype
        o = np.argsort(np.asarray(I, np.int64) * cols + np.asarray(J), kind="stable")
        self.I, self.J, self.V = np.asarray(I, np.int32)[o], np.asarray(J, np.int32)[o], V[o]

    @property
    def coo(self):
        return self.I, self.J, self.V

    def set_values(self, V):
        self.V = np.asarray(V, self.dtype)
        self.T.set_values(self.V)


def _case(pkg, ctx, name, dtype):
    """a matgen case, built with its transposed flag honoured, values salted with the specials"""
    rows, cols, I, J, V, transposed = CASES[name]
    rng = np.random.default_rng(3 + rows * 7 + cols)
    return Blk(pkg, ctx, rows, cols, I, J, _specials(rng, V), dtype, transposed)


def _rand(pkg, ctx, rng, rows, cols, fill, dtype):
    keep = np.flatnonzero(rng.random(rows * cols) < fill)
    return Blk(pkg, ctx, rows, cols, (keep // cols).astype(np.int32), (keep % cols).astype(np.int32), _specials(rng, rng.normal(size=len(keep))), dtype)


def _tilings(grid):
    return [[None if b is None else b.T for b in row] for row in grid]


def _model(grid, rs, cs, dtype):
    return concatref.concat([[None if b is None else b.coo for b in row] for row in grid], rs, cs, dtype)


def _check_readers(pkg, ctx, R, want, label):
    """mxv(transpose=True) reads vals_t, and so does step 3 of a plan that has the tiling as B"""
    rng = np.random.default_rng(5)
    x = _dev(rng.normal(size=R.rows).astype(R.dtype))
    got_y, want_y = R.mxv(x, transpose=True), want.mxv(x, transpose=True)
    z = _dev(rng.normal(size=R.cols).astype(R.dtype))
    got_z, want_z = R.mxv(z), want.mxv(z)
    ctx.synchronize()
    assert _same_numbers(got_y.cpu().numpy(), want_y.cpu().numpy()), f"{label}: mxv^T"
    assert _same_numbers(got_z.cpu().numpy(), want_z.cpu().numpy()), f"{label}: mxv"
    n = min(60, 6 * R.rows)
    key = np.sort(rng.choice(6 * R.rows, n, replace=False))
    X = pkg.Tiled.from_coo(ctx, 6, R.rows, (key // R.rows).astype(np.int32), (key % R.rows).astype(np.int32), rng.normal(size=n).astype(R.dtype),
                           dtype=R.dtype)
    pg, pw = pkg.CPlan(ctx, X, R), pkg.CPlan(ctx, X, want)
    pg.spgemm()
    pw.spgemm()
    assert all(_same_numbers(a, b) for a, b in zip(pg.export_csr(), pw.export_csr())), f"{label}: the tiling as B of a plan"


def _check(pkg, ctx, grid, rs, cs, dtype, label, explicit=True, readers=True):
    R = pkg.Tiled.concat(_tilings(grid), rs if explicit else None, cs if explicit else None)
    rows, cols, I, J, V = _model(grid, rs, cs, dtype)
    want = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=dtype)
    assert R.nnz == sum(b.T.nnz for row in grid for b in row if b is not None), label
    _assert_same_tiling(R, want, label)
    if readers:
        _check_readers(pkg, ctx, R, want, label)
    return R, want


def _unaligned_grid(pkg, ctx, rng, dtype):
    """6 x 6 blocks of the UNALIGNED sizes both ways: dense corners and strips, sparse blocks, a few nulls and empty tilings"""
    grid = []
    for a, m in enumerate(UNALIGNED):
        grid.append([])
        for b, n in enumerate(UNALIGNED):
            kind = (a * 6 + b) % 7
            grid[-1].append(None if kind == 3 else _rand(pkg, ctx, rng, m, n, (1.0, 0.5, 0.15, 0, 0.0, 0.8, 0.3)[kind], dtype))
    return grid


# ---- equality with concatref + from_coo ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", tuple(CASES))
def test_a_1x1_grid_is_a_copy(pkg, ctx, name, dtype):
    A = _case(pkg, ctx, name, dtype)
    R = pkg.Tiled.concat([[A.T]])
    _assert_same_tiling(R, A.T, name)                            # arrays equal the source's
    assert R.conv_ms > 0
    x = _dev(np.random.default_rng(5).normal(size=R.rows).astype(R.dtype))
    got, want = R.mxv(x, transpose=True), A.T.mxv(x, transpose=True)
    ctx.synchronize()
    assert _same_numbers(got.cpu().numpy(), want.cpu().numpy()), f"{name}: mxv^T"
    if name in ("ragged_37", "rect_33x65_AAt", "empty_matrix"):  # ... and the model says the same
        rows, cols, I, J, V = _model([[A]], (A.rows,), (A.cols,), dtype)
        _assert_same_tiling(R, pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=dtype), f"{name}: from_coo of the model")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_aligned_2x2(pkg, ctx, dtype):
    """all sizes multiples of 16: no shared tile, no duplicate candidate"""
    rng = np.random.default_rng(21)
    rs, cs = (48, 32), (32, 48)
    grid = [[_rand(pkg, ctx, rng, m, n, 0.1, dtype) for n in cs] for m in rs]
    R, _ = _check(pkg, ctx, grid, rs, cs, dtype, "aligned 2x2", explicit=False)
    assert R.ntiles == sum(b.T.ntiles for row in grid for b in row)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_unaligned_offsets(pkg, ctx, dtype):
    """offsets 1, 15, 16, 17 and 31 both ways: 2 x 2 cuts, result tiles fed by up to four tiles of one block and by neighbouring
    blocks, the two-tile row segment"""
    grid = _unaligned_grid(pkg, ctx, np.random.default_rng(22), dtype)
    R, _ = _check(pkg, ctx, grid, UNALIGNED, UNALIGNED, dtype, "unaligned 6x6")
    assert (R.rows, R.cols) == (64, 64)
    assert grid[5][5].T.ntiles == 9                              # the 33 x 33 block at (31, 31): each of its tiles is cut four ways


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_grid_of_1x1_blocks(pkg, ctx, dtype):
    """20 x 20 cells of 1 x 1 blocks, about half null, some empty tilings: 256 cells per result tile, 16 segments per row walk, long
    duplicate runs in the sort"""
    rng = np.random.default_rng(23)
    one = lambda: Blk(pkg, ctx, 1, 1, [0], [0], rng.choice(SPECIAL, 1), dtype)
    empty = Blk(pkg, ctx, 1, 1, [], [], [], dtype)
    shared = one()                                               # one tiling in many cells
    pick = lambda k: None if k < 10 else empty if k < 12 else shared if k < 14 else one()
    grid = [[pick(int(rng.integers(0, 20))) for _ in range(20)] for _ in range(20)]
    grid[0][0], grid[19][19], grid[16][15] = one(), one(), one()
    R, _ = _check(pkg, ctx, grid, (1,) * 20, (1,) * 20, dtype, "20x20 of 1x1")
    assert 100 < R.nnz < 260 and R.ntiles == 4


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_zero_size_strips(pkg, ctx, dtype):
    """column widths (3, 16, 1, 29, 0, 15) x row heights (0, 5, 40): a partial last tile meets the next block inside one result tile"""
    rng = np.random.default_rng(24)
    rs, cs = (0, 5, 40), (3, 16, 1, 29, 0, 15)
    grid = [[None if 0 in (m, n) else _rand(pkg, ctx, rng, m, n, 0.5, dtype) for n in cs] for m in rs]
    R, _ = _check(pkg, ctx, grid, rs, cs, dtype, "zero-size strips")
    assert (R.rows, R.cols) == (45, 64)
    grid[1][1] = grid[2][3] = None                               # ... and with holes
    _check(pkg, ctx, grid, rs, cs, dtype, "zero-size strips with holes", readers=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_null_grid_row_and_column(pkg, ctx, dtype):
    """a grid row (17 rows) and a grid column (16 columns) of only nulls: empty tile rows / columns in R"""
    rng = np.random.default_rng(25)
    rs, cs = (20, 17, 30), (25, 16, 40)
    grid = [[None if 1 in (a, b) else _rand(pkg, ctx, rng, rs[a], cs[b], 0.3, dtype) for b in range(3)] for a in range(3)]
    R, _ = _check(pkg, ctx, grid, rs, cs, dtype, "null row and column")
    assert (R.rows, R.cols) == (67, 81)
    with pytest.raises(ValueError):
        pkg.Tiled.concat(_tilings(grid))                         # the sizes of the null strips cannot be determined
    rs, cs = (32, 17, 31), (32, 16, 16)                          # ... a whole tile row and a whole tile column without tiles
    grid = [[None if 1 in (a, b) else _rand(pkg, ctx, rng, rs[a], cs[b], 0.3, dtype) for b in range(3)] for a in range(3)]
    R, _ = _check(pkg, ctx, grid, rs, cs, dtype, "an empty tile row and column", readers=False)
    assert np.diff(R.array("tile_rowptr"))[2] == 0 and np.diff(R.array("tile_colptr"))[2] == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_one_tiling_in_several_cells(pkg, ctx, dtype):
    A = _case(pkg, ctx, "ragged_37", dtype)
    R, _ = _check(pkg, ctx, [[A, A], [A, A]], (37, 37), (37, 37), dtype, "[[A, A], [A, A]]", explicit=False)
    assert R.nnz == 4 * A.T.nnz
    R, _ = _check(pkg, ctx, [[A, None], [None, A]], (37, 37), (37, 37), dtype, "[[A, 0], [0, A]]", explicit=False)
    assert R.nnz == 2 * A.T.nnz
    At = Blk(pkg, ctx, A.cols, A.rows, A.J, A.I, A.V, dtype)     # the bipartite adjacency [[0, A], [A^T, 0]]
    _check(pkg, ctx, [[None, A], [At, None]], (37, 37), (37, 37), dtype, "[[0, A], [A^T, 0]]", explicit=False, readers=False)
    RR = pkg.Tiled.concat([[R, R]])                              # a result as a block
    rows, cols, I, J, V = _model([[A, None, A, None], [None, A, None, A]], (37, 37), (37,) * 4, dtype)
    _assert_same_tiling(RR, pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=dtype), "[R R]")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_full_tiles_cut_four_ways_and_empty_candidates(pkg, ctx, dtype):
    """dense_tile at (9, 9), dense_48 at (25, 25), an empty_matrix block; a candidate that turns out empty is no tile"""
    names = ("tiny_9x9", "dense_tile", "dense_48", "empty_matrix")
    blocks = [_case(pkg, ctx, n, dtype) for n in names]
    sizes = tuple(b.rows for b in blocks)
    grid = [[blocks[a] if a == b else None for b in range(4)] for a in range(4)]
    R, _ = _check(pkg, ctx, grid, sizes, sizes, dtype, "diagonal of dense blocks")
    assert sizes == (9, 16, 48, 40) and R.nnz == 49 + 256 + 48 * 48
    grid[0][3] = _rand(pkg, ctx, np.random.default_rng(26), 9, 40, 0.0, dtype)
    _check(pkg, ctx, grid, sizes, sizes, dtype, "... beside one more empty tiling", readers=False)
    sizes = (9, 48, 40)                                          # dense_48 at (9, 9), the empty matrix after it
    grid = [[blocks[0], None, None], [None, blocks[2], None], [None, None, blocks[3]]]
    R, _ = _check(pkg, ctx, grid, sizes, sizes, dtype, "dense_48 at (9, 9)", readers=False)
    assert R.ntiles == 16 and np.diff(R.array("tile_nnz_ptr")).max() == 256
    # one entry at (3, 3) of a 5 x 5 block placed at (14, 14): its tile's box reaches four result tiles, it stores in one
    one = _case(pkg, ctx, "one_entry", dtype)
    R, _ = _check(pkg, ctx, [[None, None], [None, one]], (14, 5), (14, 5), dtype, "one entry at (17, 17)", readers=False)
    assert R.ntiles == 1 and R.array("tile_keys").tolist() == [(1 << 32) | 1]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_wide_tile_columns(pkg, ctx, dtype):
    """wide_tilecols (64 x 262 160: 16 385 tile columns) stacked on itself, and beside a 5-column block"""
    W = _case(pkg, ctx, "wide_tilecols", dtype)
    assert (W.rows, W.cols) == (64, 262_160)
    R, _ = _check(pkg, ctx, [[W], [W]], (64, 64), (262_160,), dtype, "wide on wide", explicit=False)
    assert R.tile_cols == 16_385
    five = _rand(pkg, ctx, np.random.default_rng(27), 64, 5, 0.4, dtype)
    R, _ = _check(pkg, ctx, [[W, five]], (64,), (262_160, 5), dtype, "[wide five]", explicit=False, readers=False)
    assert R.cols == 262_165 and R.array("tile_keys")[-1] & 0xFFFFFFFF == 16_385
    R, _ = _check(pkg, ctx, [[five, W]], (64,), (5, 262_160), dtype, "[five wide]", explicit=False, readers=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_hstack_and_vstack(pkg, ctx, dtype):
    rng = np.random.default_rng(28)
    hs = [_rand(pkg, ctx, rng, 21, n, 0.4, dtype) for n in (7, 30, 11)]
    R = pkg.Tiled.hstack([b.T for b in hs])
    rows, cols, I, J, V = _model([hs], (21,), (7, 30, 11), dtype)
    _assert_same_tiling(R, pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=dtype), "hstack")
    vs = [_rand(pkg, ctx, rng, m, 19, 0.4, dtype) for m in (5, 18, 40)]
    R = pkg.Tiled.vstack([b.T for b in vs])
    rows, cols, I, J, V = _model([[b] for b in vs], (5, 18, 40), (19,), dtype)
    want = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=dtype)
    _assert_same_tiling(R, want, "vstack")
    _check_readers(pkg, ctx, R, want, "vstack")
    with pytest.raises(ValueError):
        pkg.Tiled.hstack([hs[0].T, vs[0].T])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_all_blocks_empty(pkg, ctx, dtype):
    e = lambda m, n: Blk(pkg, ctx, m, n, [], [], [], dtype)
    grid = [[e(17, 5), None], [e(20, 5), e(20, 33)]]
    R, _ = _check(pkg, ctx, grid, (17, 20), (5, 33), dtype, "all empty")
    assert (R.rows, R.cols, R.nnz, R.ntiles) == (37, 38, 0, 0)
    rp, ci, v = R.export_csr()
    assert not rp.any() and len(ci) == len(v) == 0
    R.set_values_from_concat(_tilings(grid))                     # nothing to copy


# ---- refresh ---------------------------------------------------------------------------------------------------------------------------
def _refresh_grids(pkg, ctx, dtype):
    rng = np.random.default_rng(31)
    one = lambda: Blk(pkg, ctx, 1, 1, [0], [0], rng.choice(SPECIAL, 1), dtype)
    shared = one()
    pick = lambda k: None if k < 8 else shared if k < 11 else one()
    ones = [[pick(int(rng.integers(0, 20))) for _ in range(20)] for _ in range(20)]
    A = _case(pkg, ctx, "ragged_37", dtype)
    return (("20x20 of 1x1", ones, (1,) * 20, (1,) * 20), ("aliased", [[A, A], [None, A]], (37, 37), (37, 37)),
            ("unaligned", _unaligned_grid(pkg, ctx, rng, dtype), UNALIGNED, UNALIGNED))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", range(3), ids=("ones", "aliased", "unaligned"))
def test_refresh_equals_a_fresh_concat(pkg, ctx, which, dtype):
    label, grid, rs, cs = _refresh_grids(pkg, ctx, dtype)[which]
    R = pkg.Tiled.concat(_tilings(grid), rs, cs)
    rng = np.random.default_rng(41)
    X = pkg.Tiled.from_coo(ctx, 3, R.rows, np.repeat(np.arange(3, dtype=np.int32), R.rows), np.tile(np.arange(R.rows, dtype=np.int32), 3),
                           rng.normal(size=3 * R.rows).astype(dtype), dtype=dtype)
    down = pkg.CPlan(ctx, X, R)                                  # reads R's vals_t
    down.spgemm()
    sources = {id(b): b for row in grid for b in row if b is not None}
    for _ in range(2):
        for b in (b for b in sources.values() if b.T.nnz):
            b.set_values(_specials(rng, rng.normal(size=b.T.nnz)))
        R.set_values_from_concat(_tilings(grid))
        ctx.synchronize()
        F = pkg.Tiled.concat(_tilings(grid), rs, cs)
        _assert_same_tiling(R, F, f"{label}: refresh")
        assert _same_bits(R.export_csr()[2], _model(grid, rs, cs, dtype)[4]), f"{label}: the model's values (in CSR order)"
        x, z = _dev(rng.normal(size=R.rows).astype(dtype)), _dev(rng.normal(size=R.cols).astype(dtype))
        ys = [(T.mxv(z), T.mxv(x, transpose=True)) for T in (R, F)]
        ctx.synchronize()
        assert _same_numbers(ys[0][0].cpu().numpy(), ys[1][0].cpu().numpy()), f"{label}: mxv after the refresh"
        assert _same_numbers(ys[0][1].cpu().numpy(), ys[1][1].cpu().numpy()), f"{label}: mxv^T after the refresh"
        down.step3()
        fresh = pkg.CPlan(ctx, X, F)
        fresh.spgemm()
        assert all(_same_numbers(a, b) for a, b in zip(down.export_csr(), fresh.export_csr())), f"{label}: the plan after its step 3"
    R.set_values_from_concat(_tilings(grid))
    before = ctx.memory_stats()
    R.set_values_from_concat(_tilings(grid))
    assert ctx.memory_stats() == before, "a later refresh allocated"
    ctx.synchronize()
    _assert_same_tiling(R, F, f"{label}: after further refreshes")


def test_refresh_refusals(pkg, ctx):
    L = pkg.lib()
    invalid = _status(pkg, "PEM_E_INVALID")
    rng = np.random.default_rng(42)
    A, B, D = (_rand(pkg, ctx, rng, 20, 20, 0.3, np.float64) for _ in range(3))
    A2 = Blk(pkg, ctx, 20, 20, *A.coo, np.float64)               # a different tiling of equal content
    R = pkg.Tiled.concat([[A.T, B.T], [None, D.T]])
    K = pkg.Tiled.kron(A.T, B.T)
    for t, blocks in ((R, [[A.T, B.T], [None, D.T], [None, None]]),                     # a wrong count
                      (R, [[A.T, B.T, None]]),
                      (R, []),
                      (R, [[B.T, A.T], [None, D.T]]),                                   # a permuted grid of distinct tilings
                      (R, [[A.T, B.T], [D.T, None]]),
                      (R, [[A2.T, B.T], [None, D.T]]),                                  # a foreign block
                      (R, [[A.T, None], [None, D.T]]),                                  # a null where the build had a block
                      (R, [[A.T, B.T], [A.T, D.T]]),                                    # a block where the build had a null
                      (K, [[A.T, B.T]]),                                                # made by kron
                      (A.T, [[A.T]])):                                                  # not derived at all
        with pytest.raises(pkg.PemError) as e:
            t.set_values_from_concat(blocks)
        assert e.value.status == invalid
    with pytest.raises(pkg.PemError):
        R.set_values_from_kron(A.T, B.T)
    hs = (C.c_void_p * 4)(A.T._h, B.T._h, None, D.T._h)
    assert L.pem_tiled_set_values_from_concat(None, R._h, 4, hs) == invalid
    assert L.pem_tiled_set_values_from_concat(ctx._h, None, 4, hs) == invalid
    assert L.pem_tiled_set_values_from_concat(ctx._h, R._h, 4, None) == invalid
    assert L.pem_tiled_set_values_from_concat(ctx._h, R._h, -4, hs) == invalid
    assert L.pem_tiled_set_values_from_concat(ctx._h, R._h, 4, hs) == 0
    ctx.synchronize()
    _assert_same_tiling(R, pkg.Tiled.concat([[A.T, B.T], [None, D.T]]), "after the refusals")


# ---- round trip, determinism ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_split_returns_the_blocks(pkg, ctx, dtype):
    grid = _unaligned_grid(pkg, ctx, np.random.default_rng(51), dtype)
    R = pkg.Tiled.concat(_tilings(grid), UNALIGNED, UNALIGNED)
    pieces = R.split(UNALIGNED, UNALIGNED)
    for a in range(6):
        for b in range(6):
            blk = grid[a][b]
            if blk is None:
                assert (pieces[a][b].rows, pieces[a][b].cols, pieces[a][b].nnz) == (UNALIGNED[a], UNALIGNED[b], 0)
            else:
                _assert_same_tiling(pieces[a][b], blk.T, f"piece ({a}, {b})")
    back = pkg.Tiled.concat(pieces)
    _assert_same_tiling(back, R, "concat of the split")
    for rs, cs in (((64,), (63,)), ((60, 3), (64,)), ((64, 0), (64,))):
        with pytest.raises(ValueError):
            R.split(rs, cs)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_two_concats_give_identical_bytes(pkg, ctx, dtype):
    grid = _unaligned_grid(pkg, ctx, np.random.default_rng(52), dtype)
    big = [[_case(pkg, ctx, "rand_300", dtype), None], [None, _case(pkg, ctx, "powerlaw_600", dtype)]]
    for g, rs, cs in ((grid, UNALIGNED, UNALIGNED), (big, (300, 600), (300, 600))):
        R1, R2 = pkg.Tiled.concat(_tilings(g), rs, cs), pkg.Tiled.concat(_tilings(g), rs, cs)
        for name in ARRAYS:
            assert R1.array(name).tobytes() == R2.array(name).tobytes(), name
        x = _dev(np.random.default_rng(5).normal(size=R1.rows).astype(dtype))
        y1, y2 = R1.mxv(x, transpose=True), R2.mxv(x, transpose=True)
        ctx.synchronize()
        assert y1.cpu().numpy().tobytes() == y2.cpu().numpy().tobytes()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_start_no_kernel_and_leave_the_context_usable(pkg, ctx):
    L = pkg.lib()
    invalid, overflow = _status(pkg, "PEM_E_INVALID"), _status(pkg, "PEM_E_OVERFLOW")
    rng = np.random.default_rng(61)
    A, B = _rand(pkg, ctx, rng, 5, 7, 0.5, np.float64), _rand(pkg, ctx, rng, 5, 3, 0.5, np.float64)
    B32 = _rand(pkg, ctx, rng, 5, 3, 0.5, np.float32)
    tiny = Blk(pkg, ctx, 1, 1, [0], [0], [2.5], np.float64)
    other = pkg.Context(0)
    foreign = pkg.Tiled.from_coo(other, 5, 3, [1], [1], [1.0])
    h = C.c_void_p()

    def concat(gr, gc, blocks, rs, cs, out=True, c=ctx._h):
        h.value = 12345
        hs = (C.c_void_p * max(len(blocks), 1))(*[None if b is None else b._h for b in blocks]) if blocks is not None else None
        s = L.pem_tiled_concat(c, gr, gc, hs, None if rs is None else (C.c_int64 * len(rs))(*rs), None if cs is None else (C.c_int64 * len(cs))(*cs),
                               C.byref(h) if out else None)
        return s, h.value

    ctx.synchronize()
    ctx.set_kernel_profiling(True)
    ctx.reset_kernel_stats()
    before = ctx.memory_stats()
    big = 2 ** 31 - 1
    refused = (
        ("its cell", invalid, (1, 2, [A.T, B.T], [5], [7, 4])),                             # a block of the wrong shape
        ("its cell", invalid, (1, 2, [A.T, B.T], [6], [7, 3])),
        ("fp32", invalid, (1, 2, [A.T, B32.T], [5], [7, 3])),                            # mixed value types
        ("fp32", invalid, (1, 2, [B32.T, A.T], [5], [3, 7])),
        ("INT32_MAX", overflow, (2, 1, [tiny.T, None], [1, big], [1])),                  # a size sum above INT32_MAX, sizes only
        ("INT32_MAX", overflow, (1, 3, [None, tiny.T, None], [1], [big, 1, big])),
        ("INT32_MAX", overflow, (1, 2, [tiny.T, None], [1], [1, 2 ** 62])),
        ("null", invalid, (2, 2, [None] * 4, [5, 5], [7, 3])),                           # an all-null grid
        ("another context", invalid, (1, 2, [A.T, foreign], [5], [7, 3])),
        ("at least 0", invalid, (2, 1, [tiny.T, None], [1, -1], [1])),
        ("at least 1 x 1", invalid, (0, 1, [], [], [1])),
        ("at least 1 x 1", invalid, (1, -2, [], [1], [])),
    )
    for word, status, args in refused:
        assert concat(*args) == (status, None), (word, args)
        assert word in L.pem_last_error().decode(), (word, L.pem_last_error().decode())
    assert concat(1, 1, None, [1], [1]) == (invalid, None)
    assert concat(1, 1, [tiny.T], None, [1]) == (invalid, None)
    assert concat(1, 1, [tiny.T], [1], None) == (invalid, None)
    assert concat(1, 1, [tiny.T], [1], [1], c=None) == (invalid, None)
    assert concat(1, 1, [tiny.T], [1], [1], out=False)[0] == invalid
    with pytest.raises(pkg.PemError) as e:                       # the binding hands the library's refusal on
        pkg.Tiled.concat([[tiny.T, None]], col_sizes=[1, big])
    assert e.value.status == overflow
    assert ctx.kernel_stats() == {}, "a refusal started a kernel"
    assert ctx.memory_stats() == before, "a refusal allocated"
    # the context is usable: one small concat succeeds (and the check above would have seen its kernels)
    R = pkg.Tiled.concat([[A.T, B.T]])
    assert any("cc_fill" in k for k in ctx.kernel_stats())
    ctx.set_kernel_profiling(False)
    ctx.reset_kernel_stats()
    rows, cols, I, J, V = _model([[A, B]], (5,), (7, 3), np.float64)
    _assert_same_tiling(R, pkg.Tiled.from_coo(ctx, rows, cols, I, J, V), "after the refusals")
    # sizes alone make a large result: one tiny block in the far corner of 40 000 000 x 40 000 000 (candidate keys of 44 bits)
    n = 40_000_000
    R = pkg.Tiled.concat([[None, None], [None, tiny.T]], row_sizes=[n - 1, 1], col_sizes=[n - 1, 1])
    assert (R.rows, R.cols, R.nnz, R.ntiles) == (n, n, 1, 1)
    assert R.array("tile_keys").tolist() == [((n - 1) >> 4 << 32) | ((n - 1) >> 4)] and R.array("rowcolidx").tolist() == [0xFF]
    del foreign
    other.close()


# ---- CLI -------------------------------------------------------------------------------------------------------------------------------
N = 40


def _run(args, env):
    hostio = importlib.import_module("pem_spgemm_amd.hostio")
    return subprocess.run([hostio.CLI_PATH, *args], env=env, capture_output=True, text=True, timeout=120)


def _read_mtx(path):
    import scipy.io
    M = scipy.io.mmread(path).tocsr()
    M.sort_indices()
    return np.repeat(np.arange(M.shape[0], dtype=np.int32), np.diff(M.indptr)), M.indices.astype(np.int32), M.data, M.shape


@pytest.fixture
def mats(standins, tmp_path):
    rng = np.random.default_rng(71)

    def rand(r, c, nz):
        key = np.sort(rng.choice(r * c, nz, replace=False))
        return (key // c).astype(np.int32), (key % c).astype(np.int32), rng.uniform(-1, 1, nz)

    out = dict(a=rand(N, N, 200), h=rand(N, 13, 90), v=rand(21, N, 120))
    for name, shape in (("a", (N, N)), ("h", (N, 13)), ("v", (21, N))):
        out[name.upper()] = str(tmp_path / f"{name}.mtx")
        standins.write_mtx(out[name.upper()], *shape, *out[name])
    return out


def _product(oracle, mats):
    I, J, V = mats["a"]
    a = oracle.Csr(N, N, I, J, V)
    rp, ci, v = oracle.csr_spgemm(a, a).arrays()
    return np.repeat(np.arange(N, dtype=np.int32), np.diff(rp)), np.asarray(ci, np.int32), np.asarray(v)


@pytest.mark.parametrize("flag", ("--hstack", "--vstack"))
def test_cli_stacks_the_product(mats, oracle, tmp_path, flag):
    fc = str(tmp_path / "R.mtx")
    v = flag == "--vstack"
    F = mats["V" if v else "H"]
    env = dict(os.environ, PEM_CSV=str(tmp_path / "r.csv"), PEM_REPEAT="2")
    out = _run([mats["A"], "0", flag, F, "--out", fc], env)
    assert out.returncode == 0, out.stderr + out.stdout
    prod, f = _product(oracle, mats), mats["v" if v else "h"]
    want = concatref.concat([[prod], [f]], (N, 21), (N,)) if v else concatref.concat([[prod, f]], (N,), (N, 13))
    rows, cols, I, J, V = want
    assert out.stdout.count(f"{flag[2:]}: [C{';' if v else ''} {F}]") == 1 and f"{rows} x {cols}, nnz {len(I)}" in out.stdout
    gI, gJ, gV, shape = _read_mtx(fc)
    assert shape == (rows, cols) and np.array_equal(gI, I) and np.array_equal(gJ, J) and np.array_equal(gV.view(np.uint64), V.view(np.uint64))
    # the other file has the wrong row / column count: one line that names both shapes
    wrong = mats["H" if v else "V"]
    out = _run([mats["A"], "0", flag, wrong, "--out", str(tmp_path / "W.mtx")], env)
    assert out.returncode == 1, out.stdout + out.stderr
    shape_f = "40 x 13" if v else "21 x 40"
    lines = [l for l in out.stdout.splitlines() if l.startswith(flag)]
    assert lines == [f"{flag} {wrong} is {shape_f} but C is 40 x 40: the {'column' if v else 'row'} counts differ. Exiting."]
    assert not os.path.exists(str(tmp_path / "W.mtx"))
