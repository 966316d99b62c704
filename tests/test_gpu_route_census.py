"""GPU: the kernel launches of the candidate-tile route (extract.hip, kron.hip, concat.hip), of chain.hip's scatter and of the first
refresh's map kernels, counted with set_kernel_profiling / kernel_stats.  Names and counts only: what the arrays hold is the business of
the operations' own test files.  The expected counts are read from the route: one emit, one count and one fill launch per build (two emit
launches where the candidates are counted first), the candidate sort's passes in front of derive_tiled's own, nothing at all without
candidates, and a map kernel on the first refresh only."""
import numpy as np
import pytest
import torch

from hyperops import _Profiled, bits_for, derive_passes, sort_passes
from matgen import cases
from test_gpu_kron import B_SHAPES

pytestmark = pytest.mark.gpu

torch.cuda.is_available()   # (torch's runtime first, as in the other GPU files)

CASES = cases()
DTYPES = (np.float64, np.float32)
IDS = ("f64", "f32")
EX = ("ex_slots_kernel", "ex_cand_kernel", "ex_count_kernel", "ex_fill_kernel")
KR = ("kr_cand_kernel", "kr_count_kernel", "kr_fill_kernel")
CC = ("cc_cand_kernel", "cc_count_kernel", "cc_fill_kernel")


def _calls(prof, name):
    """launches of a kernel; a template's instances (ex_fill_kernel<VT>) count under its name"""
    return sum(s["calls"] for k, s in prof.stats.items() if k == name or k.startswith(name + "<"))


def _counts(prof, names):
    return tuple(_calls(prof, n) for n in names)


def _tiled(pkg, ctx, name, dtype):
    rows, cols, I, J, V, _ = CASES[name]
    return pkg.Tiled.from_coo(ctx, rows, cols, I, J, V.astype(dtype), dtype=dtype)


def _filled(pkg, ctx, rows, cols, fill, dtype, seed):
    rng = np.random.default_rng(seed)
    key = np.flatnonzero(rng.random(rows * cols) < fill)
    return pkg.Tiled.from_coo(ctx, rows, cols, (key // cols).astype(np.int32), (key % cols).astype(np.int32),
                              rng.uniform(-1.0, 1.0, len(key)).astype(dtype), dtype=dtype)


def _b_shape(pkg, ctx, name, dtype):
    """one of test_gpu_kron.py's B operands"""
    rows, cols, I, J = B_SHAPES[name]
    V = np.random.default_rng(17 + rows * 5 + cols).uniform(-1.0, 1.0, len(I))
    return pkg.Tiled.from_coo(ctx, rows, cols, I, J, V.astype(dtype), dtype=dtype)


def _empty(pkg, ctx, rows, cols, dtype):
    none = np.zeros(0, np.int32)
    return pkg.Tiled.from_coo(ctx, rows, cols, none, none, np.zeros(0, dtype), dtype=dtype)


def _route_sorts(prof, R):
    """the rs_scatter_kernel launches that are not derive_tiled's: the candidate sort's"""
    return _calls(prof, "rs_scatter_kernel") - derive_passes(R)


def _key_passes(R):
    return sort_passes(bits_for(R.tile_rows) + bits_for(R.tile_cols))


# ---- extract -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_extract_rows_one_leader(pkg, ctx, dtype):
    """I an aligned range: every output tile row reads one source tile row, so nothing is sorted"""
    A = _tiled(pkg, ctx, "ragged_37", dtype)
    with _Profiled(ctx) as prof:
        R = A.extract(rows=np.arange(16, 32))
    assert (R.rows, R.cols) == (16, 37) and R.ntiles > 1
    assert _counts(prof, EX) == (1, 1, 1, 1), prof.stats
    assert _route_sorts(prof, R) == 0, prof.stats


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("order", ("reversed", "permuted"))
def test_extract_rows_two_leaders(pkg, ctx, order, dtype):
    """37 rows in another order: an output tile row draws on two source tile rows or more, so the candidates are sorted"""
    A = _tiled(pkg, ctx, "ragged_37", dtype)
    I = np.arange(37)[::-1] if order == "reversed" else np.random.default_rng(4).permutation(37)
    with _Profiled(ctx) as prof:
        R = A.extract(rows=I)
    assert (R.rows, R.cols, R.nnz) == (37, 37, A.nnz)
    assert _counts(prof, EX) == (1, 1, 1, 1), prof.stats
    assert _route_sorts(prof, R) == _key_passes(R) == 1, prof.stats


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_extract_both_lists(pkg, ctx, dtype):
    """A(I, J) = (gather of (A(I, :))^T by J)^T: two gathers, two transposes"""
    A = _tiled(pkg, ctx, "ragged_37", dtype)
    rng = np.random.default_rng(6)
    with _Profiled(ctx) as prof:
        R = A.extract(rows=rng.permutation(37), cols=rng.permutation(37))
    assert R.nnz == A.nnz
    assert _counts(prof, EX) == (2, 2, 2, 2), prof.stats
    assert _counts(prof, ("chain_count_t_kernel", "chain_gather_t_kernel")) == (2, 2), prof.stats


# ---- kron ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_kron(pkg, ctx, dtype):
    """ragged_37 (x) s17x15: the blocks straddle tile borders, a pair reaches up to 2 x 2 tiles"""
    A, B = _tiled(pkg, ctx, "ragged_37", dtype), _b_shape(pkg, ctx, "s17x15", dtype)
    # B's tile (0, 0) holds rows 0 .. 15 and columns 0 .. 14: under A's entry (i, j) it starts at row 17 i and column 15 j of R and
    # reaches two tile rows and two tile columns where neither start is a multiple of 16 (15 j % 16 = 1 still fits one tile column)
    aI, aJ = CASES["ragged_37"][2].astype(np.int64), CASES["ragged_37"][3].astype(np.int64)
    assert np.any(((17 * aI) % 16 != 0) & ((15 * aJ) % 16 > 1)), "no candidate pair reaches 2 x 2 tiles"
    with _Profiled(ctx) as prof:
        R = pkg.Tiled.kron(A, B)
    assert (R.rows, R.cols, R.nnz) == (37 * 17, 37 * 15, A.nnz * B.nnz)
    assert _counts(prof, KR) == (2, 1, 1), prof.stats
    assert _route_sorts(prof, R) == _key_passes(R) == 2, prof.stats


# ---- concat --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("null_cell", (False, True), ids=("full", "null_cell"))
def test_concat(pkg, ctx, null_cell, dtype):
    """a 2 x 2 grid with the offsets 9 and 9: every tile of three blocks is cut and reassembled"""
    grid = [[_tiled(pkg, ctx, "tiny_9x9", dtype), _filled(pkg, ctx, 9, 37, 0.4, dtype, 7)],
            [None if null_cell else _filled(pkg, ctx, 37, 9, 0.4, dtype, 8), _tiled(pkg, ctx, "ragged_37", dtype)]]
    with _Profiled(ctx) as prof:
        R = pkg.Tiled.concat(grid, [9, 37], [9, 37])
    assert (R.rows, R.cols) == (46, 46) and R.nnz == sum(b.nnz for row in grid for b in row if b is not None)
    assert _counts(prof, CC) == (2, 1, 1), prof.stats
    assert _route_sorts(prof, R) == _key_passes(R) == 1, prof.stats


# ---- no candidates -------------------------------------------------------------------------------------------------------------------
def _nothing(R, rows, cols):
    return (R.rows, R.cols, R.nnz, R.ntiles) == (rows, cols, 0, 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_no_candidates(pkg, ctx, dtype):
    """an empty operand: the emit, count and fill stages are skipped, the result is an empty tiling of the right shape"""
    E, A = _empty(pkg, ctx, 40, 40, dtype), _tiled(pkg, ctx, "ragged_37", dtype)
    with _Profiled(ctx) as prof:
        R = E.extract(rows=[3, 1, 2, 39])
    assert _nothing(R, 4, 40)
    assert _counts(prof, EX) == (1, 0, 0, 0), prof.stats       # (the slots are what says that there are none)
    with _Profiled(ctx) as prof:
        R = pkg.Tiled.kron(A, E)
    assert _nothing(R, 37 * 40, 37 * 40)
    assert _counts(prof, KR) == (0, 0, 0), prof.stats
    with _Profiled(ctx) as prof:
        R = pkg.Tiled.concat([[E, None], [None, None]], [40, 5], [40, 3])
    assert _nothing(R, 45, 43)
    assert _counts(prof, CC) == (0, 0, 0), prof.stats
    assert _calls(prof, "rs_scatter_kernel") == 0, prof.stats


# ---- chained products ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_from_cplan(pkg, ctx, dtype):
    A = _tiled(pkg, ctx, "tiny_9x9", dtype)
    plan = pkg.CPlan(ctx, A, A)
    plan.spgemm()
    with _Profiled(ctx) as prof:
        T = pkg.Tiled.from_cplan(plan)
    assert T.nnz == plan.info()["nnz_c"] > 0
    assert _calls(prof, "chain_scatter_kernel") == 1, prof.stats


# ---- the refresh maps ----------------------------------------------------------------------------------------------------------------
def _map_calls(ctx, kernel, refresh):
    out = []
    for _ in range(2):
        with _Profiled(ctx) as prof:
            refresh()
            ctx.synchronize()
        out.append(_calls(prof, kernel))
    return tuple(out)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_map_kernels_run_once(pkg, ctx, dtype):
    """the first set_values_from_* builds the map, the second finds it"""
    A, B, S = _tiled(pkg, ctx, "ragged_37", dtype), _b_shape(pkg, ctx, "s17x15", dtype), _tiled(pkg, ctx, "tiny_9x9", dtype)
    R = A.extract(rows=np.arange(37)[::-1], cols=np.arange(3, 30))
    assert _map_calls(ctx, "ex_map_kernel", lambda: R.set_values_from_extract(A)) == (1, 0)
    K = pkg.Tiled.kron(A, B)
    assert _map_calls(ctx, "kr_map_kernel", lambda: K.set_values_from_kron(A, B)) == (1, 0)
    grid = [[S, None], [_filled(pkg, ctx, 37, 9, 0.4, dtype, 8), A]]
    G = pkg.Tiled.concat(grid)
    assert _map_calls(ctx, "cc_map_kernel", lambda: G.set_values_from_concat(grid)) == (1, 0)
    rows, cols = np.array([30, 2, 17, 16, 15, 36, 0, 8, 9]), np.array([1, 35, 16, 15, 14, 31, 32, 3, 20])
    Z = A.assign(S, rows, cols)
    assert _map_calls(ctx, "as_map_kernel", lambda: Z.set_values_from_assign(A, S)) == (1, 0)
