"""GPU: select top-k (pem_tiled_select_topk, csrc/topk.hip).

The central check: the tiling made on the device equals, array for array, the tiling pem_tiled_from_coo builds from topkref's triple of
the same matrix -- every pem_tiled_info field but the timings, all twelve arrays, values bit for bit.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import topkref as tk
from matgen import cases

pytestmark = pytest.mark.gpu

torch.cuda.is_available()   # (torch's runtime first, as in the other GPU files)

CASES = cases()
PEM_E_INVALID = -1
DTYPES = (np.float64, np.float32)
IDS = ("f64", "f32")
KS = (0, 1, 3, 16, 17, 10 ** 6)
INFO = ("rows", "cols", "nnz", "tile_rows", "tile_cols", "ntiles", "value_bytes")
ARRAYS = ("tile_keys", "tile_nnz_ptr", "masks", "rowptr", "rowcolidx", "vals", "masks_t", "tile_rowptr", "tile_colidx", "tile_colptr",
          "tile_rowidx", "tile_offsets")
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3.0e-310, 1.0e-40, 0.5, -0.5])


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32) if a.dtype.kind == "f" else a


def _assert_same_tiling(got, want, label):
    for k in INFO:
        assert getattr(got, k) == getattr(want, k), f"{label}: {k} {getattr(got, k)} != {getattr(want, k)}"
    for name in ARRAYS:
        g, w = got.array(name), want.array(name)
        assert g.dtype == w.dtype and np.array_equal(_bits(g), _bits(w)), f"{label}: array {name} differs"


def _with_specials(case, seed=3):
    """the case's values with about a fifth replaced by +-0, +-inf, NaN and subnormals (as tests/test_gpu_select.py does)"""
    rows, cols, I, J, V, _ = case
    rng = np.random.default_rng(seed + rows * 7 + cols)
    W = np.array(V, np.float64)
    sp = rng.random(len(W)) < 0.2
    W[sp] = rng.choice(SPECIAL, int(sp.sum()))
    return W


def _check(pkg, ctx, A, rows, cols, I, J, V, dtype, order, dim, k, label):
    """A.select_topk equals from_coo of topkref's triple; (I, J, V) are the entries of the rows x cols matrix A represents"""
    label = f"{label} {np.dtype(dtype).name} {order} {dim} k={k}"
    R = A.select_topk(k, order, dim)
    kept = tk.select_topk(I, J, V, order, dim, k, dtype)
    want = pkg.Tiled.from_coo(ctx, rows, cols, *kept, dtype=dtype)
    _assert_same_tiling(R, want, label)
    want.close()
    return R


def _check_all(pkg, ctx, rows, cols, I, J, V, dtype, ks, label, orders=tk.ORDERS, dims=tk.DIMS):
    V = np.asarray(V, dtype)
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=dtype)
    for order in orders:
        for dim in dims:
            for k in ks:
                _check(pkg, ctx, A, rows, cols, I, J, V, dtype, order, dim, k, label).close()
    A.close()


def _csr_coo(rp, ci, v):
    return np.repeat(np.arange(len(rp) - 1, dtype=np.int32), np.diff(rp)), np.asarray(ci, np.int32), np.asarray(v)


# ---- equality with topkref + from_coo: every matrix, dtype, order, dim and k its own test ----------------------------------------
_TILINGS = {}


def _operand(pkg, ctx, name, dtype):
    """the case's tiling (with specials) and its triple, built once per (name, dtype)"""
    key = (name, np.dtype(dtype).name)
    if key not in _TILINGS:
        rows, cols, I, J, V, _ = CASES[name]
        Vd = _with_specials(CASES[name]).astype(dtype)
        _TILINGS.clear()   # (one operand at a time: the tests of one (name, dtype) run back to back)
        _TILINGS[key] = (pkg.Tiled.from_coo(ctx, rows, cols, I, J, Vd, dtype=dtype), Vd)
    return _TILINGS[key]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("dim", tk.DIMS)
@pytest.mark.parametrize("order", tk.ORDERS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case(pkg, ctx, name, dtype, order, dim, k):
    rows, cols, I, J, _, _ = CASES[name]
    A, Vd = _operand(pkg, ctx, name, dtype)
    _check(pkg, ctx, A, rows, cols, I, J, Vd, dtype, order, dim, k, name).close()


# ---- the smallest shapes at which the kernel can still go wrong -----------------------------------------------------------------
def _maybe_t(rows, cols, I, J, transposed):
    return (cols, rows, J, I) if transposed else (rows, cols, I, J)


@pytest.mark.parametrize("transposed", (False, True), ids=("rows", "cols"))
@pytest.mark.parametrize("n", (63, 64, 65, 128, 129))
def test_trip_boundaries(pkg, ctx, n, transposed):
    """one tile row whose row 5 has n entries spread over several tiles, the other rows 0..3 entries each"""
    rng = np.random.default_rng(100 + n)
    cols = 16 * 14
    I = [np.full(n, 5)] + [np.full(r % 4, r) for r in range(16) if r != 5]
    J = [np.sort(rng.choice(cols, n, replace=False))] + [rng.choice(cols, r % 4, replace=False) for r in range(16) if r != 5]
    I, J = np.concatenate(I).astype(np.int32), np.concatenate(J).astype(np.int32)
    V = rng.uniform(-1, 1, len(I))
    V[rng.random(len(V)) < 0.1] = np.nan
    rows, cols, I, J = _maybe_t(16, cols, I, J, transposed)
    for dtype in DTYPES:
        _check_all(pkg, ctx, rows, cols, I, J, V, dtype, (1, 62, 63, 64, 65), f"trip {n}{'^T' if transposed else ''}")


def _tie_matrix(transposed):
    """16 x 1200 with 700 entries in row 3 and nothing else: the walk position of an entry is its rank by column"""
    rng = np.random.default_rng(7)
    J = np.sort(rng.choice(1200, 700, replace=False)).astype(np.int32)
    I = np.full(700, 3, np.int32)
    return _maybe_t(16, 1200, I, J, transposed)


@pytest.mark.parametrize("transposed", (False, True), ids=("rows", "cols"))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_ties_across_tiles_and_trips(pkg, ctx, dtype, transposed):
    rows, cols, I, J = _tie_matrix(transposed)
    e = np.arange(700)
    V = np.choose(e % 3, [0.5, -0.5, 0.25]).astype(dtype)
    dim = "cols" if transposed else "rows"
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=dtype)
    # the cut falls on walk position e* inside a run of equal keys: on a trip's first lane, on its last lane, mid-trip
    # (walk position = 64 * trip + lane; the positions below hold a value of the order's first class)
    first_class = {"largest": (e % 3 == 0, (192, 255, 165)), "smallest": (e % 3 == 1, (64, 319, 229)), "abs_largest": (e % 3 != 2, (64, 255, 165))}
    for order, (cls, cuts) in first_class.items():
        for at, lane in zip(cuts, (0, 63, 37)):
            assert at % 64 == lane and cls[at]
            k = int(cls[:at + 1].sum())                         # the entry at `at` is the last one kept
            R = _check(pkg, ctx, A, rows, cols, I, J, V, dtype, order, dim, k, f"ties cut at {at}")
            assert R.nnz == k
            R.close()
    for order in tk.ORDERS:   # and in the second class: everything of the first, then a cut inside 0.25's run
        for at in (128, 191, 300, 448):
            at2 = at + (2 - at % 3)   # the next 0.25
            above = (e % 3 == 0) if order == "largest" else (e % 3 == 1) if order == "smallest" else (e % 3 != 2)
            k = int(above.sum() + (e[:at2 + 1] % 3 == 2).sum())
            _check(pkg, ctx, A, rows, cols, I, J, V, dtype, order, dim, k, f"ties second class cut at {at2}").close()
    A.close()
    W = np.full(700, 0.5, dtype)
    W[::2] = np.nan                                             # ties among NaNs once the 350 numbers run out
    _check_all(pkg, ctx, rows, cols, I, J, np.full(700, 0.5), dtype, (1, 64, 65, 128, 699), "all equal", dims=(dim,))
    _check_all(pkg, ctx, rows, cols, I, J, W, dtype, (1, 64, 65, 350, 351, 414, 415), "equal and NaN", dims=(dim,))


@pytest.mark.parametrize("transposed", (False, True), ids=("rows", "cols"))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_long_line_beside_short_ones(pkg, ctx, dtype, transposed):
    """one row of 3000 entries in a 40 x 5000 matrix, its 15 tile-row neighbours holding 0, 1 and 20 entries: the fast path (the
    other tile rows for k >= 20) and the radix path in the same launch, kept and cut majors in the same wave"""
    rng = np.random.default_rng(11)
    I, J = [np.full(3000, 7)], [np.sort(rng.choice(5000, 3000, replace=False))]
    for r in range(40):
        if r != 7:
            n = (0, 1, 20)[r % 3]
            I.append(np.full(n, r))
            J.append(rng.choice(5000, n, replace=False))
    I, J = np.concatenate(I).astype(np.int32), np.concatenate(J).astype(np.int32)
    V = rng.choice(np.concatenate([SPECIAL, rng.uniform(-1, 1, 40)]), len(I))
    rows, cols, I, J = _maybe_t(40, 5000, I, J, transposed)
    _check_all(pkg, ctx, rows, cols, I, J, V, dtype, (1, 20, 21, 2999, 3000), "long line", dims=("cols" if transposed else "rows",))
    _check_all(pkg, ctx, rows, cols, I, J, V, dtype, (1, 2), "long line, the short way", orders=("largest",),
               dims=("rows" if transposed else "cols",))


def _one_row(pkg, ctx, vals, dtype, k, order):
    vals = np.asarray(vals, dtype)
    n = len(vals)
    I, J = np.zeros(n, np.int32), np.arange(n, dtype=np.int32)
    A = pkg.Tiled.from_coo(ctx, 1, n, I, J, vals, dtype=dtype)
    R = _check(pkg, ctx, A, 1, n, I, J, vals, dtype, order, "rows", k, f"row {vals.tolist()}")
    At = pkg.Tiled.from_coo(ctx, n, 1, J, I, vals, dtype=dtype)
    _check(pkg, ctx, At, n, 1, J, I, vals, dtype, order, "cols", k, f"column {vals.tolist()}").close()
    kept = R.export_csr()[1].tolist()
    for t in (A, At, R):
        t.close()
    return kept


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_key_mapping(pkg, ctx, dtype):
    dt = np.dtype(dtype)
    for order in tk.ORDERS:
        assert _one_row(pkg, ctx, [0.0, np.nan, -0.0], dtype, 2, order) == [0, 2]          # both zeros, before the NaN
        assert _one_row(pkg, ctx, [-0.0, 0.0, -0.0], dtype, 1, order) == [0]               # the zeros are equal: the lower index
        assert _one_row(pkg, ctx, [np.nan, np.nan, 1.0], dtype, 2, order) == [0, 2]        # 1.0 and the first NaN
        assert _one_row(pkg, ctx, [np.nan, 0.0, np.nan], dtype, 1, order) == [1]           # a zero ranks strictly above a NaN
        assert _one_row(pkg, ctx, [np.nan, -np.inf, np.nan, np.inf], dtype, 2, order) == [1, 3]
    tiny = 5e-324 if dt == np.float64 else 1e-45   # the smallest subnormal
    assert dt.type(tiny) > 0
    v = [-np.inf, np.inf, tiny, -tiny, 0.0]
    want = dict(largest=[1, 2, 4, 3, 0], smallest=[0, 3, 4, 2, 1], abs_largest=[0, 1, 2, 3, 4])
    for order in tk.ORDERS:
        for k in range(1, 6):
            assert _one_row(pkg, ctx, v, dtype, k, order) == sorted(want[order][:k]), (order, k)
    one = dt.type(1.0)
    up, down = np.nextafter(one, dt.type(2)), np.nextafter(one, dt.type(0))               # the lowest mantissa bit
    assert _one_row(pkg, ctx, [one, up, down, -up, -one], dtype, 1, "largest") == [1]
    assert _one_row(pkg, ctx, [one, up, down, -up, -one], dtype, 2, "largest") == [0, 1]
    assert _one_row(pkg, ctx, [one, up, down, -up, -one], dtype, 1, "smallest") == [3]
    assert _one_row(pkg, ctx, [one, up, down, -up, -one], dtype, 2, "abs_largest") == [1, 3]
    assert _one_row(pkg, ctx, [one, up, down, -up, -one], dtype, 3, "abs_largest") == [0, 1, 3]
    assert _one_row(pkg, ctx, [-2.5, 2.5, -2.5], dtype, 1, "largest") == [1]              # only the sign bit differs
    assert _one_row(pkg, ctx, [2.5, -2.5, 2.5], dtype, 1, "smallest") == [1]
    assert _one_row(pkg, ctx, [-2.5, 2.5, -2.5], dtype, 2, "abs_largest") == [0, 1]
    # NaNs of every payload and sign rank alike, below -inf: by index among themselves
    u = np.uint64 if dt == np.float64 else np.uint32
    payloads = np.array([0xFFF8000000000001, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF] if dt == np.float64 else [0xFFC00001, 0x7F800001, 0xFFFFFFFF], u)
    nans = payloads.view(dtype)
    assert np.isnan(nans).all()
    mixed = np.full(4, -np.inf, dtype)
    mixed[[0, 2, 3]] = nans                                     # (copied bit for bit)
    for order in tk.ORDERS:
        assert _one_row(pkg, ctx, mixed, dtype, 1, order) == [1]
        assert _one_row(pkg, ctx, mixed, dtype, 3, order) == [0, 1, 2]
        assert _one_row(pkg, ctx, nans[::-1].copy(), dtype, 2, order) == [0, 1]


def test_empties(pkg, ctx):
    E = pkg.Tiled.from_coo(ctx, 40, 40, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    for order in tk.ORDERS:
        for dim in tk.DIMS:
            for k in (0, 1, 10 ** 6):
                Z = E.select_topk(k, order, dim)
                assert Z.nnz == 0 and Z.ntiles == 0 and (Z.rows, Z.cols) == (40, 40)
    # empty rows and empty tile rows between full ones
    rng = np.random.default_rng(5)
    I, J = np.meshgrid(np.r_[0:16, 17, 48:64, 100], np.arange(70), indexing="ij")
    I, J = I.ravel().astype(np.int32), J.ravel().astype(np.int32)
    V = rng.uniform(-1, 1, len(I))
    for dtype in DTYPES:
        _check_all(pkg, ctx, 120, 70, I, J, V, dtype, (0, 1, 33, 34, 35, 69, 70, 71), "empty rows between full ones")
    A = pkg.Tiled.from_coo(ctx, 120, 70, I, J, V)
    X = A.select_topk(0)
    assert X.nnz == 0 and X.ntiles == 0 and (X.rows, X.cols) == (120, 70)
    rp, ci, v = X.export_csr()
    assert np.array_equal(rp, np.zeros(121, np.int32)) and len(ci) == len(v) == 0
    assert X.select_topk(3, "smallest", "cols").nnz == 0
    for order in tk.ORDERS:
        for dim in tk.DIMS:
            _assert_same_tiling(A.select_topk(70 if dim == "rows" else 34, order, dim), A, f"k = the longest line, {order} {dim}")
            _assert_same_tiling(A.select_topk(2 ** 62, order, dim), A, f"k = 2^62, {order} {dim}")


# ---- every tiling is an operand -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ("rand_300", "rect_70x40_AAt", "rect_33x65_AAt", "ragged_37", "powerlaw_600", "dense_48"))
def test_transposed_tiling_is_filtered_as_its_matrix(pkg, ctx, name, dtype):
    """a tiling built with transpose = 1 represents M^T: top-k works on M^T's rows and columns"""
    rows, cols, I, J, V, _ = CASES[name]
    Vd = _with_specials(CASES[name]).astype(dtype)
    T = pkg.Tiled.from_coo(ctx, rows, cols, I, J, Vd, True, dtype=dtype)
    assert (T.rows, T.cols) == (cols, rows)
    for order in tk.ORDERS:
        for dim in tk.DIMS:
            for k in (1, 3, 17):
                _check(pkg, ctx, T, cols, rows, J, I, Vd, dtype, order, dim, k, f"{name}^T").close()


@pytest.mark.parametrize("how", ("from_cplan", "ewise", "select", "transpose", "kron"))
def test_derived_operands(pkg, ctx, how):
    rows, cols, I, J, V, _ = CASES["rand_50"]
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    if how == "from_cplan":
        p = pkg.CPlan(ctx, A, A)
        p.spgemm()
        D = pkg.Tiled.from_cplan(p)
    elif how == "ewise":
        D = pkg.Tiled.ewise(A, A.transpose(), "plus")
    elif how == "select":
        D = A.select("abs_gt", 0.2)
    elif how == "transpose":
        D = A.transpose()
    else:
        B = pkg.Tiled.from_coo(ctx, 2, 3, np.array([0, 1, 1], np.int32), np.array([2, 0, 1], np.int32), np.array([1.0, -2.0, 0.5]))
        D = pkg.Tiled.kron(A, B)
    dI, dJ, dV = _csr_coo(*D.export_csr())
    for order, dim, k in (("largest", "rows", 3), ("abs_largest", "cols", 2), ("smallest", "cols", 17), ("smallest", "rows", 1)):
        _check(pkg, ctx, D, D.rows, D.cols, dI, dJ, dV, np.float64, order, dim, k, how)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_result_works_downstream(pkg, oracle, ctx, dtype):
    rows, cols, I, J, V, _ = CASES["powerlaw_600"]
    f32 = dtype == np.float32
    o = np.argsort(I.astype(np.int64) * cols + J, kind="stable")
    I, J, V = I[o], J[o], np.asarray(V, dtype)[o]
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=dtype)
    for order, dim, k in (("largest", "cols", 4), ("abs_largest", "rows", 3)):
        R = A.select_topk(k, order, dim)
        kI, kJ, kV = tk.select_topk(I, J, V, order, dim, k, dtype)
        rp, ci, v = R.export_csr()
        assert np.array_equal(rp, np.r_[0, np.cumsum(np.bincount(kI, minlength=rows))]) and np.array_equal(ci, kJ)
        assert np.array_equal(_bits(v), _bits(kV))
        p = pkg.CPlan(ctx, R, R)                                # R . R against the oracle
        p.spgemm()
        orr = oracle.Csr(rows, cols, kI, kJ, kV.astype(np.float64))
        got, want = p.export_csr(), oracle.csr_spgemm(orr, orr, f32=f32).arrays()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), f"{order} {dim}: structure of R.R"
        assert np.array_equal(_bits(got[2]), _bits(np.asarray(want[2]).astype(dtype))), f"{order} {dim}: values of R.R"
        _assert_same_tiling(R.select_topk(k, order, dim), R, f"{order} {dim}: idempotent")
        _assert_same_tiling(R.select_topk(k + 1, order, dim), R, f"{order} {dim}: k + 1 of a top-k result")
        want_t = pkg.Tiled.from_coo(ctx, rows, cols, kI, kJ, kV, dtype=dtype)
        for d in tk.DIMS:
            y, yw = R.reduce("plus", d), want_t.reduce("plus", d)
            ctx.synchronize()
            assert torch.equal(y, yw), f"{order} {dim}: reduce {d}"
        # entries per line of dim, through the tiling itself: at most k
        ones = pkg.Tiled.from_coo(ctx, rows, cols, kI, kJ, np.ones(len(kI), dtype), dtype=dtype)
        count, count_w = R.apply("one").reduce("plus", dim), ones.reduce("plus", dim)
        ctx.synchronize()
        assert torch.equal(count, count_w) and float(count.max()) == k


def test_mcl_iteration_as_documented(pkg):
    """INTEGRATION.md section 3q's Markov-clustering iteration, as written there (on a context that shares torch's stream, so the
    column sums need no extra synchronisation)"""
    rows, cols, I, J, V, _ = CASES["rand_300"]
    prev, st = torch.cuda.current_stream(), torch.cuda.Stream()
    torch.cuda.set_stream(st)
    ctx = pkg.Context(0, stream=st.cuda_stream)
    try:
        M = pkg.Tiled.from_coo(ctx, rows, cols, I, J, np.abs(V) + 0.01)
        eps, k = 1e-4, 5
        plan = pkg.CPlan(ctx, M, M); plan.spgemm()                         # expansion M^2
        E = pkg.Tiled.from_cplan(plan).apply("powi", 2)                    # inflation x -> x^2
        s = E.reduce("plus", "cols")                                       # column sums
        M = E.scale(cols=1.0 / s).select("abs_gt", eps)                    # column normalisation, then the drop
        pI, pJ, pV = _csr_coo(*M.export_csr())
        M = M.select_topk(k, "largest", "cols")                            # selection by rank
        want = pkg.Tiled.from_coo(ctx, rows, cols, *tk.select_topk(pI, pJ, pV, "largest", "cols", k))
        _assert_same_tiling(M, want, "MCL iteration")
        assert 0 < M.nnz < len(pI) and np.bincount(_csr_coo(*M.export_csr())[1], minlength=cols).max() == k
        for t in (want, M, E, plan):
            t.close()
    finally:
        ctx.close()
        torch.cuda.set_stream(prev)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_two_calls_give_identical_arrays(pkg, ctx, dtype):
    rows, cols, I, J, _, _ = CASES["hub_row_4000"]
    Vd = _with_specials(CASES["hub_row_4000"]).astype(dtype)
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, Vd, dtype=dtype)
    for order in tk.ORDERS:
        for dim in tk.DIMS:
            R1, R2 = A.select_topk(5, order, dim), A.select_topk(5, order, dim)
            _assert_same_tiling(R1, R2, f"{order} {dim}: two calls")


@pytest.mark.parametrize("first", tk.DIMS)
def test_schedule_built_mid_life(pkg, ctx, first):
    """the column call after a row call on the same tiling, and the reverse: the column schedule is built on the first column call"""
    rows, cols, I, J, _, _ = CASES["band_1500"]
    Vd = _with_specials(CASES["band_1500"])
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, Vd)
    second = "cols" if first == "rows" else "rows"
    for dim in (first, second, first, second):
        for k in (2, 9):
            _check(pkg, ctx, A, rows, cols, I, J, Vd, np.float64, "abs_largest", dim, k, f"{first} first").close()
    y = A.reduce("plus", "cols")                                  # the schedule serves reduce as one built by reduce does
    yw = pkg.Tiled.from_coo(ctx, rows, cols, I, J, Vd).reduce("plus", "cols")
    ctx.synchronize()
    assert np.array_equal(_bits(y.cpu().numpy()), _bits(yw.cpu().numpy()))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments(pkg, ctx):
    L = pkg.lib()
    rows, cols, I, J, V, _ = CASES["rand_50"]
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    marker = 0x1234
    h = C.c_void_p(marker)

    def call(a, order, dim, k, out=True, c=ctx._h):
        return L.pem_tiled_select_topk(c, a, order, dim, C.c_int64(k), C.byref(h) if out else None)

    ctx.synchronize()
    before = ctx.memory_stats()
    for args in ((A._h, 0, 0, -1), (A._h, 0, 0, -(2 ** 63)), (A._h, 3, 0, 1), (A._h, -1, 0, 1), (A._h, 0, 2, 1), (A._h, 0, -1, 1), (None, 0, 0, 1)):
        assert call(*args) == PEM_E_INVALID, args
        assert h.value == marker, f"{args}: *out changed"
        assert b"pem_tiled_select_topk" in L.pem_last_error(), args
    assert call(A._h, 0, 0, 1, out=False) == PEM_E_INVALID
    assert call(A._h, 0, 0, 1, c=None) == PEM_E_INVALID
    assert ctx.memory_stats() == before, "refused without allocating"
    assert call(A._h, 2, 1, 0) == 0 and h.value != marker
    pkg.Tiled(ctx, h).close()
    for kwargs in (dict(k=-1), dict(k=1.5), dict(k=1, order="biggest"), dict(k=1, dim="diag")):
        with pytest.raises(ValueError):
            A.select_topk(**kwargs)
    assert A.select_topk(np.int64(2)).nnz == A.select_topk(2.0).nnz


def test_no_refresh(pkg, ctx):
    rows, cols, I, J, V, _ = CASES["rand_300"]
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    for dim in tk.DIMS:
        R = A.select_topk(10 ** 6, "largest", dim)               # (even where nothing was dropped)
        with pytest.raises(pkg.PemError) as e:
            R.set_values_from_select(A)
        assert e.value.status == PEM_E_INVALID and "pem_tiled_set_values_from_select" in str(e.value)


@pytest.mark.parametrize("dim", tk.DIMS)
def test_intermediates_go_back_to_the_arena(pkg, ctx, dim):
    rows, cols, I, J, V, _ = CASES["powerlaw_600"]
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    A.select("value_ne", 7.0).close()                            # (the context's own temporaries grow to this size once,
    A.select_topk(10 ** 6, "largest", dim).close()               # and the column schedule stays with A from here on)
    ctx.synchronize()
    before = ctx.memory_stats()["in_use_bytes"]
    Q = A.select("value_ne", 7.0)                                # what a select result that keeps everything holds
    q = ctx.memory_stats()["in_use_bytes"] - before
    Q.close()
    assert q > 0 and ctx.memory_stats()["in_use_bytes"] == before
    R = A.select_topk(10 ** 6, "largest", dim)
    assert ctx.memory_stats()["in_use_bytes"] - before == q, "the build left more in use than the result's own arrays"
    R.close()
    for k in (0, 2, 40):
        A.select_topk(k, "abs_largest", dim).close()
    assert ctx.memory_stats()["in_use_bytes"] == before, "a closed result left memory in use"
