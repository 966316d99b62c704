"""GPU: the Kronecker product (pem_tiled_kron) and its refresh (pem_tiled_set_values_from_kron).

The central check: the tiling made on the device equals, array for array, the tiling pem_tiled_from_coo builds from kronref's entries
-- every pem_tiled_info field but the timings, all twelve arrays, values bit for bit (NaN equals NaN; zeros may differ in sign for
min / max).  vals_t is no pem_tiled_array: it is checked through its readers, mxv(transpose=True) and step 3's B side.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import frontierref
import kronref
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


def _status(pkg, name):
    return {v: k for k, v in pkg.STATUS_NAMES.items()}[name]


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32) if a.dtype.kind == "f" else a


def _same_vals(got, want, op="times"):
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    nan = np.isnan(got) & np.isnan(want)
    exact = _bits(got) == _bits(want)
    if op in ("min", "max"):
        exact |= (got == 0) & (want == 0)
    return bool(np.all(exact | nan))


def _assert_same_tiling(got, want, label, op="times"):
    for k in INFO:
        assert getattr(got, k) == getattr(want, k), f"{label}: {k} {getattr(got, k)} != {getattr(want, k)}"
    for name in ARRAYS:
        g, w = got.array(name), want.array(name)
        if name == "vals":
            assert _same_vals(g, w, op), f"{label}: vals differ"
        else:
            assert np.array_equal(g, w), f"{label}: array {name} differs"


def _same_results(xs, ys, op="times"):
    return all(_same_vals(x, y, op) if np.asarray(x).dtype.kind == "f" else np.array_equal(x, y) for x, y in zip(xs, ys))


def _canonical(I, J, V, cols):
    o = np.argsort(np.asarray(I, np.int64) * cols + np.asarray(J), kind="stable")
    return np.asarray(I, np.int32)[o], np.asarray(J, np.int32)[o], np.asarray(V)[o]


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


class Op:
    """an operand: the tiling and the canonical entries of the matrix it represents"""

    def __init__(self, pkg, ctx, rows, cols, I, J, V, dtype, transposed=False):
        V = np.asarray(V, dtype)
        self.T = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, bool(transposed), dtype=dtype)
        if transposed:                                           # a tiling built with transpose = 1 is the tiling of its own matrix
            rows, cols, I, J = cols, rows, J, I
        self.rows, self.cols = rows, cols
        self.I, self.J, self.V = _canonical(I, J, V, cols)
        self.dtype = dtype

    @property
    def coo(self):
        return self.rows, self.cols, self.I, self.J, self.V


def _a_operand(pkg, ctx, name, dtype, specials=True):
    """a matgen case, built with its transposed flag honoured, values salted with the specials"""
    rows, cols, I, J, V, transposed = CASES[name]
    rng = np.random.default_rng(3 + rows * 7 + cols)
    return Op(pkg, ctx, rows, cols, I, J, _specials(rng, V) if specials else V, dtype, transposed)


def _filled(rng, rows, cols, fill):
    keep = rng.random(rows * cols) < fill
    key = np.flatnonzero(keep)
    return (key // cols).astype(np.int32), (key % cols).astype(np.int32)


def _b_shapes():
    """name -> (rows, cols, I, J): the smallest shapes that hit each boundary of the walk"""
    rng = np.random.default_rng(2024)
    dense = lambda r, c: tuple(x.ravel().astype(np.int32) for x in np.meshgrid(np.arange(r), np.arange(c), indexing="ij"))
    out = {}
    out["b1x1"] = (1, 1) + dense(1, 1)                              # a pattern copy
    out["dense2"] = (2, 2) + dense(2, 2)                            # divides 16; up to 64 A entries per tile; duplicate candidates
    out["dense3"] = (3, 3) + dense(3, 3)
    I, J = dense(3, 5)
    holes = ~np.isin(I * 5 + J, (1, 7, 8, 13))
    out["holes3x5"] = (3, 5, I[holes], J[holes])                   # divides nothing; blocks straddle tile borders both ways
    out["dense16"] = (16, 16) + dense(16, 16)                       # aligned; one pair per tile
    out["s17x15"] = (17, 15) + _filled(rng, 17, 15, 0.6)            # straddle by one row, short by one column
    out["s32x48"] = (32, 48) + _filled(rng, 32, 48, 0.3)            # aligned, several B tiles
    r, c, I, J, _, _ = CASES["ragged_37"]
    out["ragged_37"] = (r, c, I, J)                                 # B tile clipped at the edge
    out["row1x40"] = (1, 40) + _filled(rng, 1, 40, 0.5)
    out["col40x1"] = (40, 1) + _filled(rng, 40, 1, 0.5)
    out["empty40"] = (40, 40, np.zeros(0, np.int32), np.zeros(0, np.int32))
    return out


B_SHAPES = _b_shapes()
assert len(B_SHAPES["s17x15"][2]) and B_SHAPES["s17x15"][2].max() == 16 and B_SHAPES["s32x48"][3].max() >= 32


def _b_operand(pkg, ctx, name, dtype, specials=True):
    rows, cols, I, J = B_SHAPES[name]
    rng = np.random.default_rng(17 + rows * 5 + cols)
    V = rng.uniform(-1.0, 1.0, len(I))
    return Op(pkg, ctx, rows, cols, I, J, _specials(rng, V) if specials else V, dtype)


def _want(pkg, ctx, A, B, op, dtype):
    rows, cols, I, J, V = kronref.kron(*A.coo, *B.coo, op, dtype)
    return (rows, cols, I, J, V), pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=dtype)


def _check_vals_t(ctx, R, want, label, op="times"):
    """mxv(transpose=True) reads vals_t"""
    x = _dev(np.random.default_rng(5).normal(size=R.rows).astype(R.dtype))
    got_y, want_y = R.mxv(x, transpose=True), want.mxv(x, transpose=True)
    ctx.synchronize()
    assert _same_vals(got_y.cpu().numpy(), want_y.cpu().numpy(), op), f"{label}: mxv^T"


def _check_kron(pkg, ctx, A, B, op, label, dtype):
    R = pkg.Tiled.kron(A.T, B.T, op)
    coo, want = _want(pkg, ctx, A, B, op, dtype)
    assert R.nnz == A.T.nnz * B.T.nnz, label
    _assert_same_tiling(R, want, label, op)
    _check_vals_t(ctx, R, want, label, op)
    return R, coo, want


# every A with three or four Bs; every B shape and every A at least twice
PAIRS = dict(
    one_entry=("b1x1", "dense16", "s17x15", "empty40"),
    tiny_9x9=("dense2", "holes3x5", "ragged_37", "row1x40"),
    ragged_37=("holes3x5", "s17x15", "s32x48", "col40x1"),
    dense_tile=("dense3", "dense2", "dense16", "holes3x5"),
    rect_33x65_AAt=("b1x1", "s32x48", "ragged_37", "row1x40"),
    empty_rows=("dense2", "s17x15", "col40x1"),
    empty_matrix=("dense16", "holes3x5", "empty40", "ragged_37"),
    row_vector_AAt=("dense2", "s32x48", "col40x1", "row1x40"),
    col_vector_AAt=("holes3x5", "dense16", "row1x40", "b1x1"),
    cancel_and_zero=("b1x1", "s17x15", "empty40", "col40x1"),
    rand_300=("dense2", "holes3x5", "dense16", "s32x48"),           # the multi-workgroup case
)


def test_the_pairs_cover_every_shape_twice():
    used = [b for bs in PAIRS.values() for b in bs]
    for b in B_SHAPES:
        assert used.count(b) >= (1 if b == "dense3" else 2), b
    assert all(3 <= len(bs) <= 4 for bs in PAIRS.values())


# ---- equality with kronref + from_coo ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", tuple(PAIRS))
def test_kron_equals_from_coo_of_the_model(pkg, ctx, name, dtype):
    A = _a_operand(pkg, ctx, name, dtype)
    for bname in PAIRS[name]:
        B = _b_operand(pkg, ctx, bname, dtype)
        R, coo, want = _check_kron(pkg, ctx, A, B, "times", f"{name} (x) {bname}", dtype)
        assert (R.rows, R.cols) == (A.rows * B.rows, A.cols * B.cols)
        if (name, bname) == ("dense_tile", "dense3"):
            assert R.ntiles == 9 and np.array_equal(np.diff(R.array("tile_nnz_ptr")), np.full(9, 256)), "nine full tiles"
        if bname == "b1x1":                                         # a pattern copy
            for arr in ("tile_keys", "tile_nnz_ptr", "rowcolidx", "masks"):
                assert np.array_equal(R.array(arr), A.T.array(arr)), arr
        if 0 in (A.T.nnz, B.T.nnz):
            assert R.nnz == 0 and R.ntiles == 0
            rp, ci, v = R.export_csr()
            assert not rp.any() and len(ci) == len(v) == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name,bname", (("ragged_37", "s17x15"), ("rect_33x65_AAt", "holes3x5")))
def test_every_op(pkg, ctx, name, bname, dtype):
    A, B = _a_operand(pkg, ctx, name, dtype), _b_operand(pkg, ctx, bname, dtype)
    for op in kronref.BINOPS:
        _check_kron(pkg, ctx, A, B, op, f"{name} (x) {bname} under {op}", dtype)
    for bad in ("minus", "pair", None):
        with pytest.raises(ValueError):
            pkg.Tiled.kron(A.T, B.T, bad)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_result_as_the_b_operand_of_a_product(pkg, ctx, dtype):
    """step 3 reads B's vals_t"""
    rng = np.random.default_rng(9)
    for name, bname, op in (("ragged_37", "s17x15", "times"), ("rand_300", "holes3x5", "plus"), ("tiny_9x9", "ragged_37", "max")):
        A, B = _a_operand(pkg, ctx, name, dtype), _b_operand(pkg, ctx, bname, dtype)
        R = pkg.Tiled.kron(A.T, B.T, op)
        _, want = _want(pkg, ctx, A, B, op, dtype)
        key = np.sort(rng.choice(20 * R.rows, 300, replace=False))
        X = pkg.Tiled.from_coo(ctx, 20, R.rows, (key // R.rows).astype(np.int32), (key % R.rows).astype(np.int32),
                               rng.normal(size=300).astype(dtype), dtype=dtype)
        for sr in ("plus_times", "min_plus"):
            pg, pw = pkg.CPlan(ctx, X, R, semiring=sr), pkg.CPlan(ctx, X, want, semiring=sr)
            pg.spgemm()
            pw.spgemm()
            assert _same_results(pg.export_csr(), pw.export_csr(), op), f"{name} (x) {bname} {op}: R as B under {sr}"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_same_handle_and_derived_operands(pkg, ctx, dtype):
    import selectref
    A = _a_operand(pkg, ctx, "ragged_37", dtype)
    _check_kron(pkg, ctx, A, A, "times", "ragged_37 (x) itself", dtype)
    # a derived A (a select result) and a derived B (a transpose)
    S = A.T.select("triu", 1)
    sI, sJ, sV = selectref.select(A.I, A.J, A.V, "triu", 1, dtype)
    B = _b_operand(pkg, ctx, "s17x15", dtype)
    R = pkg.Tiled.kron(S, B.T)
    rows, cols, I, J, V = kronref.kron(A.rows, A.cols, sI, sJ, sV, *B.coo, "times", dtype)
    _assert_same_tiling(R, pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=dtype), "select (x) B")
    Bt = B.T.transpose()
    R = pkg.Tiled.kron(S, Bt, "plus")
    rows, cols, I, J, V = kronref.kron(A.rows, A.cols, sI, sJ, sV, B.cols, B.rows, B.J, B.I, B.V, "plus", dtype)
    want = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=dtype)
    _assert_same_tiling(R, want, "select (x) transpose", "plus")
    _check_vals_t(ctx, R, want, "select (x) transpose", "plus")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name,bname", (("rect_33x65_AAt", "s17x15"), ("tiny_9x9", "holes3x5"), ("empty_rows", "col40x1")))
def test_transpose_of_the_product_is_the_product_of_the_transposes(pkg, ctx, name, bname, dtype):
    A, B = _a_operand(pkg, ctx, name, dtype), _b_operand(pkg, ctx, bname, dtype)
    for op in ("times", "min"):
        left = pkg.Tiled.kron(A.T, B.T, op).transpose()
        right = pkg.Tiled.kron(A.T.transpose(), B.T.transpose(), op)
        _assert_same_tiling(left, right, f"{name} (x) {bname} {op}", op)
        _check_vals_t(ctx, left, right, f"{name} (x) {bname} {op}", op)


def test_results_feed_other_operations_and_round_trip(pkg, ctx, tmp_path):
    """save / load, select, another kron, and the tensor-product operator A (x) I + I (x) B by one ewise"""
    import ewiseref
    import selectref
    dtype = np.float64
    A, B = _a_operand(pkg, ctx, "tiny_9x9", dtype, specials=False), _b_operand(pkg, ctx, "holes3x5", dtype, specials=False)
    R, (rows, cols, I, J, V), _ = _check_kron(pkg, ctx, A, B, "times", "tiny (x) holes", dtype)
    assert R.conv_ms > 0
    path = str(tmp_path / "k.pemtile")
    R.save(path)
    _assert_same_tiling(pkg.Tiled.load(ctx, path), R, "save / load")
    s = selectref.select(I, J, V, "abs_gt", 0.25, dtype)
    _assert_same_tiling(R.select("abs_gt", 0.25), pkg.Tiled.from_coo(ctx, rows, cols, *s), "kron -> select")
    RR = pkg.Tiled.kron(R, B.T, "plus")
    r2 = kronref.kron(rows, cols, I, J, V, *B.coo, "plus", dtype)
    _assert_same_tiling(RR, pkg.Tiled.from_coo(ctx, *r2), "kron -> kron", "plus")
    # A (x) I_m + I_n (x) S for square A (n x n) and S (m x m)
    S = _a_operand(pkg, ctx, "cancel_and_zero", dtype, specials=False)
    n, m = A.rows, S.rows
    eye = lambda k: (k, k, np.arange(k, dtype=np.int32), np.arange(k, dtype=np.int32), np.ones(k))
    In, Im = Op(pkg, ctx, *eye(n), dtype), Op(pkg, ctx, *eye(m), dtype)
    L = pkg.Tiled.ewise(pkg.Tiled.kron(A.T, Im.T), pkg.Tiled.kron(In.T, S.T), "plus")
    k1, k2 = kronref.kron(*A.coo, *Im.coo, "times", dtype), kronref.kron(*In.coo, *S.coo, "times", dtype)
    e = ewiseref.ewise(n * m, k1[2:], k2[2:], "plus")
    _assert_same_tiling(L, pkg.Tiled.from_coo(ctx, n * m, n * m, *e), "A (x) I + I (x) S", "plus")


# ---- Kronecker power -------------------------------------------------------------------------------------------------------------------
def test_kronecker_power_and_bfs_on_it(pkg, ctx):
    """a 3 x 3 seed with 5 entries raised to the 6th power by repeated kron of results: 729 x 729, 15 625 entries"""
    dtype = np.float64
    sI, sJ = np.array([0, 0, 1, 2, 2], np.int32), np.array([0, 1, 2, 0, 2], np.int32)
    sV = np.array([0.9, 0.7, 0.6, 0.8, 0.5])
    seed = Op(pkg, ctx, 3, 3, sI, sJ, sV, dtype)
    K, model = seed.T, seed.coo
    for _ in range(5):
        K = pkg.Tiled.kron(K, seed.T)
        model = kronref.kron(*model, *seed.coo, "times", dtype)
    rows, cols, I, J, V = model
    assert (K.rows, K.cols, K.nnz) == (729, 729, 15_625) == (rows, cols, len(I))
    _assert_same_tiling(K, pkg.Tiled.from_coo(ctx, rows, cols, I, J, V), "seed^6")
    rp = np.concatenate([[0], np.cumsum(np.bincount(I, minlength=rows))]).astype(np.int64)
    for src in (0, 364, 728):
        for tr in (False, True):
            lv, depth, reached = K.bfs(src, transpose=tr)
            want, wdepth, wreached = frontierref.bfs(rows, rp, J.astype(np.int64), src, tr)
            torch.cuda.synchronize()
            assert np.array_equal(lv.cpu().numpy(), want) and (depth, reached) == (wdepth, wreached), (src, tr)
    assert frontierref.bfs(rows, rp, J.astype(np.int64), 0)[2] > 1


# ---- wide indices ----------------------------------------------------------------------------------------------------------------------
def _scattered(rng, n, count):
    """a few dozen entries of an n x n matrix, both corners and both sides of a tile border among them"""
    pinned = np.array([0, 15 * n + 16, 16 * n + 15, (n - 1) * n + (n - 1), (n - 1) * n, n - 1], np.int64)
    key = np.unique(np.concatenate([pinned, rng.choice(n * n, count, replace=False)]))
    return (key // n).astype(np.int32), (key % n).astype(np.int32), rng.normal(size=len(key))


def test_wide_indices(pkg, ctx):
    """3000 x 3000 (x) 2800 x 2800: 8 400 000 rows and columns, more than 2^19 tile rows"""
    dtype = np.float64
    rng = np.random.default_rng(31)
    A = Op(pkg, ctx, 3000, 3000, *_scattered(rng, 3000, 40), dtype)
    B = Op(pkg, ctx, 2800, 2800, *_scattered(rng, 2800, 36), dtype)
    R, (rows, cols, I, J, V), want = _check_kron(pkg, ctx, A, B, "times", "wide", dtype)
    assert rows == 8_400_000 and R.tile_rows > 2 ** 19 and I.max() == rows - 1 and J.max() == cols - 1
    rp, ci, v = R.export_csr()
    assert np.array_equal(np.repeat(np.arange(rows, dtype=np.int32), np.diff(rp)), I) and np.array_equal(ci, J) and _same_vals(v, V)
    x = _dev(rng.normal(size=cols))
    y, yw = R.mxv(x), want.mxv(x)
    ctx.synchronize()
    assert _same_vals(y.cpu().numpy(), yw.cpu().numpy())
    A.T.set_values(rng.normal(size=A.T.nnz))
    B.T.set_values(rng.normal(size=B.T.nnz))
    R.set_values_from_kron(A.T, B.T)
    ctx.synchronize()
    F = pkg.Tiled.kron(A.T, B.T)
    _assert_same_tiling(R, F, "wide refresh")
    _check_vals_t(ctx, R, F, "wide refresh")


# ---- refresh ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name,bname,op", (("ragged_37", "s17x15", "times"), ("rect_33x65_AAt", "holes3x5", "plus"), ("rand_300", "s32x48", "min")))
def test_refresh_equals_a_fresh_product(pkg, ctx, name, bname, op, dtype):
    A, B = _a_operand(pkg, ctx, name, dtype), _b_operand(pkg, ctx, bname, dtype)
    R = pkg.Tiled.kron(A.T, B.T, op)
    rng = np.random.default_rng(41)
    for which in ("A", "B", "both"):
        if which in ("A", "both"):
            A.T.set_values(_specials(rng, rng.normal(size=A.T.nnz)))
        if which in ("B", "both"):
            B.T.set_values(_specials(rng, rng.normal(size=B.T.nnz)))
        R.set_values_from_kron(A.T, B.T)
        ctx.synchronize()
        F = pkg.Tiled.kron(A.T, B.T, op)
        _assert_same_tiling(R, F, f"{name} (x) {bname} {op}: refresh after new values of {which}", op)
        _check_vals_t(ctx, R, F, f"{name} (x) {bname} {op}: refresh after new values of {which}", op)
    before = ctx.memory_stats()["block_allocs"]
    R.set_values_from_kron(A.T, B.T)
    R.set_values_from_kron(A.T, B.T)
    assert ctx.memory_stats()["block_allocs"] == before, "a later refresh allocated"
    ctx.synchronize()


def test_second_refresh_allocates_nothing(pkg, ctx):
    A, B = _a_operand(pkg, ctx, "tiny_9x9", np.float64), _b_operand(pkg, ctx, "dense2", np.float64)
    R = pkg.Tiled.kron(A.T, B.T)
    R.set_values_from_kron(A.T, B.T)                            # the first call builds the map
    before = ctx.memory_stats()
    R.set_values_from_kron(A.T, B.T)
    after = ctx.memory_stats()
    assert (after["block_allocs"], after["in_use_bytes"]) == (before["block_allocs"], before["in_use_bytes"])
    ctx.synchronize()
    _assert_same_tiling(R, pkg.Tiled.kron(A.T, B.T), "after two refreshes")


def test_refresh_refusals(pkg, ctx):
    L = pkg.lib()
    invalid = _status(pkg, "PEM_E_INVALID")
    A, B = _a_operand(pkg, ctx, "tiny_9x9", np.float64), _b_operand(pkg, ctx, "dense2", np.float64)
    A2 = _a_operand(pkg, ctx, "tiny_9x9", np.float64)           # a different tiling of equal content
    R = pkg.Tiled.kron(A.T, B.T)
    Q = pkg.Tiled.kron(A.T, A.T)
    E = pkg.Tiled.ewise(A.T, A.T)
    for t, a, b in ((R, B.T, A.T), (R, A2.T, B.T), (R, A.T, A.T), (E, A.T, A.T), (A.T, A.T, B.T), (Q, A.T, A2.T)):
        with pytest.raises(pkg.PemError) as e:
            t.set_values_from_kron(a, b)
        assert e.value.status == invalid
    with pytest.raises(pkg.PemError):
        R.set_values_from_ewise(A.T, B.T)                       # made by kron
    assert L.pem_tiled_set_values_from_kron(None, R._h, A.T._h, B.T._h) == invalid
    assert L.pem_tiled_set_values_from_kron(ctx._h, None, A.T._h, B.T._h) == invalid
    assert L.pem_tiled_set_values_from_kron(ctx._h, R._h, None, B.T._h) == invalid
    assert L.pem_tiled_set_values_from_kron(ctx._h, R._h, A.T._h, None) == invalid
    R.set_values_from_kron(A.T, B.T)
    Q.set_values_from_kron(A.T, A.T)
    ctx.synchronize()
    _assert_same_tiling(Q, pkg.Tiled.kron(A.T, A.T), "same handle refresh")


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg, ctx):
    L = pkg.lib()
    invalid, overflow = _status(pkg, "PEM_E_INVALID"), _status(pkg, "PEM_E_OVERFLOW")
    A = _a_operand(pkg, ctx, "tiny_9x9", np.float64)
    A32 = _a_operand(pkg, ctx, "tiny_9x9", np.float32)
    h = C.c_void_p()

    def kron(a, b, op, out=True, c=ctx._h):
        h.value = 12345
        s = L.pem_tiled_kron(c, a, b, op, C.byref(h) if out else None)
        return s, h.value

    assert kron(A.T._h, A32.T._h, 1) == (invalid, None)         # mixed value types
    assert kron(A32.T._h, A.T._h, 1) == (invalid, None)
    for op in (-1, 6, 100):
        assert kron(A.T._h, A.T._h, op) == (invalid, None), op
    assert kron(None, A.T._h, 1) == (invalid, None)
    assert kron(A.T._h, None, 1) == (invalid, None)
    assert kron(A.T._h, A.T._h, 1, c=None) == (invalid, None)
    assert kron(A.T._h, A.T._h, 1, out=False)[0] == invalid
    with pytest.raises(pkg.PemError) as e:
        pkg.Tiled.kron(A.T, A32.T)
    assert e.value.status == invalid
    # dimensions: 65 536 * 65 536 = 2^32
    one = lambda: pkg.Tiled.from_coo(ctx, 65_536, 65_536, [40_000], [3], [2.5])
    P, Q = one(), one()
    # entries: the dimensions fit (46 341^2 = 2 147 488 281 > INT32_MAX only as an entry count ... and 46 341 x 46 341 as a shape)
    n = 46_341
    col = pkg.Tiled.from_coo(ctx, n, 1, np.arange(n, dtype=np.int32), np.zeros(n, np.int32), np.ones(n))
    row = pkg.Tiled.from_coo(ctx, 1, n, np.zeros(n, np.int32), np.arange(n, dtype=np.int32), np.ones(n))
    ctx.synchronize()
    for a, b, word in ((P, Q, "dimension"), (col, row, "entries")):
        before = ctx.memory_stats()
        assert kron(a._h, b._h, 1) == (overflow, None), word
        assert word in L.pem_last_error().decode()
        assert ctx.memory_stats() == before, f"{word}: refused without allocating"
    # ... while the same operands the other way round are fine where they fit: 1 x n (x) n x 1 is n x n with n^2 entries -- too many
    # as well; a slice of them is not
    few = pkg.Tiled.from_coo(ctx, 1, n, np.zeros(3, np.int32), np.array([0, 7, n - 1], np.int32), np.ones(3))
    R = pkg.Tiled.kron(col, few)
    assert (R.rows, R.cols, R.nnz) == (n, n, 3 * n)
    rp, ci, v = R.export_csr()
    assert np.array_equal(np.diff(rp), np.full(n, 3)) and np.array_equal(ci.reshape(n, 3), np.tile([0, 7, n - 1], (n, 1)))
