"""GPU: tilings built from triplets with duplicates (pem_tiled_build*, csrc/build.hip) and their refresh
(pem_tiled_set_values_from_build).

The central check is test_gpu_kron.py's: the tiling made on the device equals, array for array, the tiling pem_tiled_from_coo builds
from buildref.fold's entries -- every pem_tiled_info field but the timings, all twelve arrays, values bit for bit (NaN equals NaN;
zeros may differ in sign for min / max).  vals_t is no pem_tiled_array: it is checked through mxv(transpose=True) and a plan's B side.

Fold order: a run of at most BUILD_INORDER_MAX duplicates is folded strictly left to right, so every op is bit-exact against
buildref.  A longer run keeps the order but may be regrouped: min, max, lor, land, first and second do not depend on the grouping,
plus is exact on small integers and times on +-1 with a single 3; plus on standard-normal values is held to the bound on two
differently grouped sums of the same n values, |got - ref| <= 2 g sum|v| with g = (n - 1) u / (1 - (n - 1) u), u the unit roundoff
(each grouping is within g sum|v| of the exact sum; Higham, Accuracy and Stability of Numerical Algorithms, section 4.2).
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import buildref
from matgen import cases

pytestmark = pytest.mark.gpu

torch.cuda.is_available()   # (torch's runtime first, as in the other GPU files)

CASES = cases()
DTYPES = (np.float64, np.float32)
IDS = ("f64", "f32")
OPS = buildref.DUP_OPS
GROUPING_FREE = ("min", "max", "lor", "land", "first", "second")
INFO = ("rows", "cols", "nnz", "tile_rows", "tile_cols", "ntiles", "value_bytes")
ARRAYS = ("tile_keys", "tile_nnz_ptr", "masks", "rowptr", "rowcolidx", "vals", "masks_t", "tile_rowptr", "tile_colidx", "tile_colptr",
          "tile_rowidx", "tile_offsets")
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3.0e-310, 1.0e-40, 0.5, -0.5])   # (test_gpu_kron.py's)
TRANSPOSED = ("rect_33x65_AAt", "rect_70x40_AAt")
BOTH_ENTRY_POINTS = "rand_300"


def _status(pkg, name):
    return {v: k for k, v in pkg.STATUS_NAMES.items()}[name]


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32) if a.dtype.kind == "f" else a


def _same(got, want, op):
    """elementwise: the same bits, NaN for NaN, or (min / max) zeros of either sign"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape
    ok = (_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))
    if op in ("min", "max"):
        ok |= (got == 0) & (want == 0)
    return ok


def _assert_same_tiling(got, want, label, op, vals=True):
    for k in INFO:
        assert getattr(got, k) == getattr(want, k), f"{label}: {k} {getattr(got, k)} != {getattr(want, k)}"
    for name in ARRAYS:
        g, w = got.array(name), want.array(name)
        if name == "vals":
            assert not vals or bool(np.all(_same(g, w, op))), f"{label}: vals differ"
        else:
            assert np.array_equal(g, w), f"{label}: array {name} differs"


def _dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()   # (the arrays are read on the context's stream)
    return t


def _check_vals_t(ctx, R, want, label, op):
    """mxv(transpose=True) reads vals_t"""
    x = _dev(np.random.default_rng(5).normal(size=R.rows).astype(R.dtype))
    got_y, want_y = R.mxv(x, transpose=True), want.mxv(x, transpose=True)
    ctx.synchronize()
    assert bool(np.all(_same(got_y.cpu().numpy(), want_y.cpu().numpy(), op))), f"{label}: mxv^T"


def _want(pkg, ctx, rows, cols, I, J, V, op, dtype, transpose=False):
    oI, oJ, oV = buildref.fold(rows, cols, I, J, V, op, transpose)
    r, c = (cols, rows) if transpose else (rows, cols)
    return (oI, oJ, oV), pkg.Tiled.from_coo(ctx, r, c, oI, oJ, oV, dtype=dtype)


def _build_device(pkg, ctx, rows, cols, I, J, V, op, dtype, transpose=False, keep_map=False):
    dI, dJ, dV = _dev(np.asarray(I, np.int32)), _dev(np.asarray(J, np.int32)), _dev(np.asarray(V, dtype))
    return pkg.Tiled.build_device(ctx, rows, cols, len(I), dI.data_ptr(), dJ.data_ptr(), dV.data_ptr(), dup=op, transpose=transpose, dtype=dtype,
                                  keep_map=keep_map)


# ---- 1. every matgen case, run lengths 1 to 5 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(CASES))
def test_build_equals_from_coo_of_the_fold(pkg, ctx, name):
    rows, cols, I, J, V, _ = CASES[name]
    rng = np.random.default_rng(100 + rows + 3 * cols)
    tI, tJ, tV64 = buildref.with_duplicates(I, J, V, rng, rng.integers(1, 6, len(I)))
    transpose = name in TRANSPOSED
    for dtype in DTYPES:
        tV = tV64.astype(dtype)
        for op in OPS:
            label = f"{name} {op} {np.dtype(dtype).name}"
            got = pkg.Tiled.build(ctx, rows, cols, tI, tJ, tV, dup=op, transpose=transpose, dtype=dtype)
            (oI, _, _), want = _want(pkg, ctx, rows, cols, tI, tJ, tV, op, dtype, transpose)
            assert got.nnz == len(oI) == len(I), label
            _assert_same_tiling(got, want, label, op)
            if op in ("plus", "second"):
                _check_vals_t(ctx, got, want, label, op)
            if name == BOTH_ENTRY_POINTS:
                _assert_same_tiling(_build_device(pkg, ctx, rows, cols, tI, tJ, tV, op, dtype, transpose), want, label + " (device)", op)


# ---- 2. stream edges ------------------------------------------------------------------------------------------------------------------
def _tiled_order(I, J, tile_cols):
    return np.lexsort((J & 15, I & 15, J >> 4, I >> 4))   # (tile row, tile column, r, c): the sort key of the route


def _edge_lengths(T):
    """run lengths in sorted order: T-1, T, T+1, 64, 65 and 257, runs across the sorted positions 63|64 and 255|256, the first run at
    0 and (any list has that) the last run ending at nnz_in - 1"""
    L = [T - 1]
    pad = lambda p: L.extend([1] * max(0, p - sum(L)))
    pad(63)
    L += [T, T + 1]
    pad(255)
    L += [64, 65, 2, 3, 5, 1, 1, 257]
    start = np.concatenate([[0], np.cumsum(L)])
    for p in (63, 255):   # some run holds positions p and p + 1
        k = np.searchsorted(start, p, side="right") - 1
        assert start[k] <= p and start[k + 1] > p + 1, (T, p)
    return np.array(L)


def _edge_input(pkg, kind, dtype, seed=7):
    """(I, J, V, length of every fold's run in canonical order) on a 40 x 40 matrix (3 x 3 tiles, ragged edge)"""
    T = pkg.BUILD_INORDER_MAX
    rng = np.random.default_rng(seed)
    L = _edge_lengths(T)
    key = rng.choice(40 * 40, size=len(L), replace=False)
    I, J = (key // 40).astype(np.int32), (key % 40).astype(np.int32)
    o = _tiled_order(I, J, 3)
    I, J = I[o], J[o]                                          # entry k is the k-th run of the sorted stream
    rep = np.repeat(np.arange(len(L)), L)
    n = len(rep)
    if kind == "ints":
        V = rng.integers(-4, 5, n).astype(dtype)
    elif kind == "pm1":                                        # +-1, and a single 3 in every run longer than T
        V = rng.choice([-1.0, 1.0], n).astype(dtype)
        first = np.concatenate([[0], np.cumsum(L)[:-1]])
        for k in np.flatnonzero(L > T):
            V[first[k] + rng.integers(0, L[k])] = 3
    else:
        V = rng.normal(size=n).astype(dtype)
    p = rng.permutation(n)
    tI, tJ, tV = I[rep][p], J[rep][p], V[p]
    canon = np.argsort(I.astype(np.int64) * 40 + J)            # fold's order
    return tI, tJ, tV, L[canon]


def _plus_bound(rows, cols, I, J, V, dtype):
    """per entry of the fold: 2 g sum|v| over its run, in float64"""
    order, start, _ = buildref.runs(rows, cols, I, J)
    n = np.diff(start).astype(np.float64)
    u = 2.0 ** -53 if np.dtype(dtype) == np.float64 else 2.0 ** -24
    g = (n - 1) * u / (1 - (n - 1) * u)
    return 2 * g * np.add.reduceat(np.abs(np.asarray(V, np.float64)[order]), start[:-1])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_stream_edges(pkg, ctx, dtype):
    T = pkg.BUILD_INORDER_MAX
    for kind, ops in (("ints", OPS), ("pm1", ("times",)), ("normal", OPS)):
        tI, tJ, tV, runlen = _edge_input(pkg, kind, dtype)
        order, start, _ = buildref.runs(40, 40, tI, tJ)
        assert start[0] == 0 and start[-1] == len(tI) and {T - 1, T, T + 1, 64, 65, 257} <= set(runlen.tolist())
        for op in ops:
            label = f"{kind} {op}"
            got = pkg.Tiled.build(ctx, 40, 40, tI, tJ, tV, dup=op, dtype=dtype)
            (_, _, oV), want = _want(pkg, ctx, 40, 40, tI, tJ, tV, op, dtype)
            _assert_same_tiling(got, want, label, op, vals=False)
            # (a 40 x 40 tiling stores its tiles' entries row-major per tile: compare in canonical order through the export)
            gv, wv = got.export_csr()[2], want.export_csr()[2]
            assert np.array_equal(_bits(wv), _bits(oV))
            same = _same(gv, wv, op)
            short = runlen <= T
            assert bool(np.all(same[short])), f"{label}: a run of at most {T} is not bit-exact"
            exact_long = op in GROUPING_FREE or (kind == "ints" and op == "plus") or (kind == "pm1" and op == "times")
            if exact_long:
                assert bool(np.all(same)), f"{label}: a long run differs"
                _check_vals_t(ctx, got, want, label, op)
            elif op == "plus":
                err = np.abs(gv.astype(np.float64) - wv.astype(np.float64))
                bound = _plus_bound(40, 40, tI, tJ, tV, dtype)
                print(f"{label} {np.dtype(dtype).name}: max err / bound over the long runs = {np.max(err[~short] / bound[~short]):.3g}")
                assert bool(np.all(err <= bound)), f"{label}: beyond the regrouping bound"


# ---- 3. one position 5000 times -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", ((1, 1, 0, 0), (33, 17, 32, 16)), ids=("1x1", "33x17"))
def test_one_position_5000_times(pkg, ctx, shape, dtype):
    rows, cols, i, j = shape
    n = 5000
    rng = np.random.default_rng(31)
    I, J = np.full(n, i, np.int32), np.full(n, j, np.int32)
    pm1 = rng.choice([-1.0, 1.0], n).astype(dtype)
    pm1[1234] = 3
    for kind, V, ops in (("ints", rng.integers(-4, 5, n).astype(dtype), OPS), ("pm1", pm1, ("times",)), ("normal", rng.normal(size=n).astype(dtype), OPS)):
        for op in ops:
            got = pkg.Tiled.build(ctx, rows, cols, I, J, V, dup=op, dtype=dtype)
            (_, _, oV), want = _want(pkg, ctx, rows, cols, I, J, V, op, dtype)
            assert got.nnz == 1 and got.ntiles == 1
            _assert_same_tiling(got, want, f"{kind} {op}", op, vals=False)
            gv = got.array("vals")
            if op in GROUPING_FREE or (kind == "ints" and op == "plus") or (kind == "pm1" and op == "times"):
                assert bool(np.all(_same(gv, oV, op))), (kind, op, gv, oV)
            elif op == "plus":
                assert abs(float(gv[0]) - float(oV[0])) <= _plus_bound(rows, cols, I, J, V, dtype)[0], (kind, op, gv, oV)


# ---- 4. degenerate inputs -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_degenerate_inputs(pkg, ctx, dtype):
    rows, cols, I, J, V, _ = CASES["ragged_37"]
    V = V.astype(dtype)
    dI, dJ, dV = _dev(I), _dev(J), _dev(V)
    plain = pkg.Tiled.from_coo_device(ctx, rows, cols, len(I), dI.data_ptr(), dJ.data_ptr(), dV.data_ptr(), dtype=dtype)
    for op in OPS:   # duplicate-free: pem_tiled_from_coo_device's tiling, whatever the op
        got = pkg.Tiled.build_device(ctx, rows, cols, len(I), dI.data_ptr(), dJ.data_ptr(), dV.data_ptr(), dup=op, dtype=dtype)
        _assert_same_tiling(got, plain, f"duplicate-free {op}", "times")
        _check_vals_t(ctx, got, plain, f"duplicate-free {op}", "times")
    none = np.zeros(0, np.int32)
    empty = pkg.Tiled.build(ctx, 40, 23, none, none, np.zeros(0, dtype), dup="plus", dtype=dtype, keep_map=True)
    assert (empty.nnz, empty.ntiles, empty.rows, empty.cols) == (0, 0, 40, 23)
    _assert_same_tiling(empty, pkg.Tiled.from_coo(ctx, 40, 23, none, none, np.zeros(0, dtype), dtype=dtype), "empty", "plus")
    empty.set_values_from_build(0, nnz_in=0)
    ctx.synchronize()
    for op in OPS:
        one = pkg.Tiled.build(ctx, 40, 23, [39], [22], np.array([-0.0], dtype), dup=op, dtype=dtype)
        _assert_same_tiling(one, pkg.Tiled.from_coo(ctx, 40, 23, [39], [22], np.array([-0.0], dtype), dtype=dtype), f"single {op}", "times")


# ---- 5. wide keys: five sort passes ---------------------------------------------------------------------------------------------------
def test_wide_keys_keep_the_input_order(pkg, ctx):
    n = 70_000                                                   # 4375 tile rows and columns: 13 + 13 + 8 = 34 key bits
    rng = np.random.default_rng(51)
    key = rng.choice(n * n, size=1400, replace=False)
    key = np.concatenate([key, key[rng.integers(0, 1400, 600)]])
    key = key[rng.permutation(len(key))]
    I, J = (key // n).astype(np.int32), (key % n).astype(np.int32)
    V = np.arange(len(key), dtype=np.float64) + 1                # every triplet its own value: a swapped pair shows
    for op in ("first", "second"):
        for dtype in DTYPES:
            got = pkg.Tiled.build(ctx, n, n, I, J, V.astype(dtype), dup=op, dtype=dtype)
            (oI, _, _), want = _want(pkg, ctx, n, n, I, J, V.astype(dtype), op, dtype)
            assert got.nnz == len(oI) < len(key) - 400
            _assert_same_tiling(got, want, f"wide {op}", op)


# ---- 6. specials among the duplicates -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_specials_among_the_duplicates(pkg, ctx, dtype):
    rows, cols, I, J, _, _ = CASES["ragged_37"]
    rng = np.random.default_rng(61)
    V = rng.choice(SPECIAL, len(I)).astype(dtype)
    tI, tJ, tV = buildref.with_duplicates(I, J, V, rng, rng.integers(1, 6, len(I)))
    for op in OPS:
        got = pkg.Tiled.build(ctx, rows, cols, tI, tJ, tV, dup=op, dtype=dtype)
        _, want = _want(pkg, ctx, rows, cols, tI, tJ, tV, op, dtype)
        _assert_same_tiling(got, want, f"specials {op}", op)


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------------
def test_errors(pkg, ctx):
    invalid = _status(pkg, "PEM_E_INVALID")
    V = np.ones(3)
    for I, J in (([0, 40, 1], [0, 0, 1]), ([0, 1, 2], [0, -1, 2]), ([0, 1, 2], [0, 23, 2])):
        with pytest.raises(pkg.PemError) as e:
            pkg.Tiled.build(ctx, 40, 23, I, J, V)
        assert e.value.status == invalid and "index out of range for a 40 x 23 matrix" in str(e.value)
    I = np.array([0, 1, 0], np.int32)
    h = C.c_void_p()
    for bad in (-1, 8, 99):
        s = pkg.lib().pem_tiled_build(ctx._h, 4, 4, C.c_int64(3), I.ctypes.data_as(C.c_void_p), I.ctypes.data_as(C.c_void_p),
                                      V.ctypes.data_as(C.c_void_p), 0, bad, 0, C.byref(h))
        assert s == invalid and not h.value
        assert f"unknown op {bad} (a pem_binop 0 .. 5, PEM_DUP_FIRST = 6 or PEM_DUP_SECOND = 7)" in pkg.lib().pem_last_error().decode()
    with pytest.raises(pkg.PemError) as e:                       # the entry points that refuse duplicates still do
        pkg.Tiled.from_coo(ctx, 4, 4, I, I, V)
    assert e.value.status == _status(pkg, "PEM_E_DUPLICATE") and "duplicate (row, col) entries in the input" in str(e.value)


# ---- 8. refresh -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_refresh_equals_a_fresh_build_and_allocates_nothing(pkg, ctx, oracle, dtype):
    f32 = np.dtype(dtype) == np.float32
    tI, tJ, tV, _ = _edge_input(pkg, "normal", dtype)            # long and short runs, 40 x 40
    rng = np.random.default_rng(81)
    state = _status(pkg, "PEM_E_STATE")
    for op in ("plus", "max", "second"):
        t = pkg.Tiled.build(ctx, 40, 40, tI, tJ, tV, dup=op, dtype=dtype, keep_map=True)
        plan = pkg.CPlan(ctx, t, t)                              # reads vals and, on the B side, vals_t
        plan.spgemm()
        for trip in range(3):
            newV = rng.normal(size=len(tI)).astype(dtype)
            if op == "plus" and trip == 2:                       # small integers: the long runs' sums are exact under any grouping,
                newV = rng.integers(-4, 5, len(tI)).astype(dtype)   # so the plan below can be held to the serial oracle
            dV = _dev(newV)                                      # (kept alive until the context's stream has read it)
            before = ctx.memory_stats()
            t.set_values_from_build(dV)
            after = ctx.memory_stats()
            if trip:                                             # (the first refresh may allocate: vmap_t, the sorted values)
                assert all(after[k] == before[k] for k in ("driver_allocs", "block_allocs")), f"{op}: refresh {trip + 1} allocated"
            ctx.synchronize()
            fresh = pkg.Tiled.build(ctx, 40, 40, tI, tJ, newV, dup=op, dtype=dtype)
            _assert_same_tiling(t, fresh, f"refresh {op}", "times")   # bit for bit, whatever the op
            _check_vals_t(ctx, t, fresh, f"refresh {op}", "times")
        with pytest.raises(pkg.PemError) as e:                   # the plan on t is stale until its step 3
            plan.export_csr()
        assert e.value.status == state
        plan.spgemm()
        rp, ci, v = plan.export_csr()
        oI, oJ, oV = buildref.fold(40, 40, tI, tJ, newV, op)
        oa = oracle.Csr(40, 40, oI, oJ, np.asarray(oV, np.float64))
        rp0, ci0, v0 = oracle.csr_spgemm(oa, oa, f32=f32).arrays()
        assert np.array_equal(rp, rp0) and np.array_equal(ci, ci0) and np.array_equal(v, np.asarray(v0, dtype)), op


def test_refresh_refusals_and_what_a_tiling_keeps(pkg):
    ctx = pkg.Context(0)                                         # (its own context: the memory figures are this test's alone)
    invalid = _status(pkg, "PEM_E_INVALID")
    rows, cols, I, J, V, _ = CASES["ragged_37"]
    rng = np.random.default_rng(82)
    tI, tJ, tV = buildref.with_duplicates(I, J, V, rng, rng.integers(1, 6, len(I)))
    dV = _dev(tV)
    oI, oJ, oV = buildref.fold(rows, cols, tI, tJ, tV, "plus")

    def own_bytes(make):
        """the device memory the tiling itself holds: what its destruction gives back"""
        t = make()
        with_t = ctx.memory_stats()["in_use_bytes"]
        t.close()
        return with_t - ctx.memory_stats()["in_use_bytes"]

    plain = own_bytes(lambda: pkg.Tiled.from_coo(ctx, rows, cols, oI, oJ, oV))
    built = own_bytes(lambda: pkg.Tiled.build(ctx, rows, cols, tI, tJ, tV))
    kept = own_bytes(lambda: pkg.Tiled.build(ctx, rows, cols, tI, tJ, tV, keep_map=True))
    assert 0 < built <= plain < kept
    t = pkg.Tiled.build(ctx, rows, cols, tI, tJ, tV)
    with pytest.raises(pkg.PemError) as e:
        t.set_values_from_build(dV)
    assert e.value.status == invalid and "was not made by pem_tiled_build with PEM_BUILD_KEEP_MAP" in str(e.value)
    t = pkg.Tiled.build(ctx, rows, cols, tI, tJ, tV, keep_map=True)
    with pytest.raises(pkg.PemError) as e:
        t.set_values_from_build(dV.data_ptr(), nnz_in=len(tI) - 1)
    assert e.value.status == invalid and f"from {len(tI) - 1} triplets" in str(e.value)
    with pytest.raises(pkg.PemError) as e:                       # a plain tiling
        pkg.Tiled.from_coo(ctx, rows, cols, oI, oJ, oV).set_values_from_build(dV)
    assert e.value.status == invalid
    t.set_values_from_build(dV)                                  # the right call still works; every other refresh does too
    ctx.synchronize()
    assert np.array_equal(_bits(t.export_csr()[2]), _bits(oV))
    t.set_values(oV[::-1].copy())
    ctx.synchronize()
    assert np.array_equal(t.export_csr()[2], oV[::-1])
    ctx.close()


# ---- 9. determinism -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_two_builds_are_bitwise_equal(pkg, ctx, dtype):
    tI, tJ, tV, _ = _edge_input(pkg, "normal", dtype)
    for op in ("plus", "times"):
        a = pkg.Tiled.build(ctx, 40, 40, tI, tJ, tV, dup=op, dtype=dtype)
        b = _build_device(pkg, ctx, 40, 40, tI, tJ, tV, op, dtype)
        for name in ARRAYS:
            assert np.array_equal(_bits(a.array(name)), _bits(b.array(name))), (op, name)


# ---- 10. past the scan's level boundary -----------------------------------------------------------------------------------------------
def test_four_million_triplets_equal_scipys_sum(pkg, ctx):
    n, nnz_in = 65_536, 4_200_000
    rng = np.random.default_rng(101)
    pos = rng.choice(n * n, size=1_000_000, replace=False)
    key = pos[rng.integers(0, len(pos), nnz_in)]                 # about 1 M distinct positions (nearly all of pos), mean run 4.2
    I, J = (key // n).astype(np.int32), (key % n).astype(np.int32)
    V = rng.integers(-4, 5, nnz_in).astype(np.float64)           # exact sums in any order
    t = pkg.Tiled.build(ctx, n, n, I, J, V)
    M = sp.coo_matrix((V, (I, J)), shape=(n, n))
    M.sum_duplicates()
    M = M.tocsr()
    M.sort_indices()
    assert 900_000 < t.nnz == M.nnz
    rp, ci, v = t.export_csr()
    assert np.array_equal(rp, M.indptr) and np.array_equal(ci, M.indices) and np.array_equal(v, M.data)


# ---- 11. the built tiling as an operand -----------------------------------------------------------------------------------------------
def test_a_built_tiling_is_an_operand(pkg, ctx, oracle):
    rows, cols, I, J, V, _ = CASES["rand_300"]
    rng = np.random.default_rng(111)
    tI, tJ, tV = buildref.with_duplicates(I, J, V, rng, rng.integers(1, 6, len(I)))
    oI, oJ, oV = buildref.fold(rows, cols, tI, tJ, tV, "plus")
    A = pkg.Tiled.build(ctx, rows, cols, tI, tJ, tV)
    want = pkg.Tiled.from_coo(ctx, rows, cols, oI, oJ, oV)
    plan = pkg.CPlan(ctx, A, A)
    plan.spgemm()
    oa = oracle.Csr(rows, cols, oI, oJ, oV)
    for got, ref in zip(plan.export_csr(), oracle.csr_spgemm(oa, oa).arrays()):
        assert np.array_equal(got, ref)
    _assert_same_tiling(A.transpose(), want.transpose(), "transpose", "times")
    _assert_same_tiling(pkg.Tiled.ewise(A, A), pkg.Tiled.ewise(want, want), "ewise", "times")
    _assert_same_tiling(A.select("tril"), want.select("tril"), "select", "times")
