"""GPU: select (pem_tiled_select) and its positional refresh (pem_tiled_set_values_from_select).

The central check: the tiling made on the device equals, array for array, the tiling pem_tiled_from_coo builds from selectref's COO of
the same matrix -- every pem_tiled_info field but the timings, all twelve arrays, values bit for bit.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import selectref as sel
from matgen import cases

pytestmark = pytest.mark.gpu

torch.cuda.is_available()   # (torch's runtime first, as in the other GPU files)

CASES = cases()
PEM_E_INVALID = -1
DTYPES = (np.float64, np.float32)
INFO = ("rows", "cols", "nnz", "tile_rows", "tile_cols", "ntiles", "value_bytes")
ARRAYS = ("tile_keys", "tile_nnz_ptr", "masks", "rowptr", "rowcolidx", "vals", "masks_t", "tile_rowptr", "tile_colidx", "tile_colptr",
          "tile_rowidx", "tile_offsets")
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3.0e-310, 1.0e-40, 0.5, -0.5])
THUNKS = {op: (0, -1, 3) for op in sel.POSITIONAL}
THUNKS.update({op: (0.0, 0.25, -0.5) for op in sel.OPS[8:]})


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32) if a.dtype.kind == "f" else a


def _same_vals(got, want, op="plus"):
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    nan = np.isnan(got) & np.isnan(want)
    exact = _bits(got) == _bits(want)
    if op in ("min", "max"):
        exact |= (got == 0) & (want == 0)
    return bool(np.all(exact | nan))


def _assert_same_tiling(got, want, label, op="plus"):
    for k in INFO:
        assert getattr(got, k) == getattr(want, k), f"{label}: {k} {getattr(got, k)} != {getattr(want, k)}"
    for name in ARRAYS:
        g, w = got.array(name), want.array(name)
        if name == "vals":
            assert _same_vals(g, w, op), f"{label}: vals differ"
        else:
            assert np.array_equal(g, w), f"{label}: array {name} differs"


def _canonical(I, J, V, cols):
    o = np.argsort(np.asarray(I, np.int64) * cols + np.asarray(J), kind="stable")
    return np.asarray(I, np.int32)[o], np.asarray(J, np.int32)[o], np.asarray(V)[o]


def _with_specials(case, seed=3):
    """the case's values with about a fifth replaced by +-0, +-inf, NaN and subnormals"""
    rows, cols, I, J, V, _ = case
    rng = np.random.default_rng(seed + rows * 7 + cols)
    W = np.array(V, np.float64)
    sp = rng.random(len(W)) < 0.2
    W[sp] = rng.choice(SPECIAL, int(sp.sum()))
    return W


def _expect(pkg, ctx, rows, cols, I, J, V, op, thunk, dtype):
    """from_coo of selectref's result; (I, J) are coordinates of the rows x cols matrix the tiling represents"""
    kI, kJ, kV = sel.select(I, J, V, op, thunk, dtype)
    return pkg.Tiled.from_coo(ctx, rows, cols, kI, kJ, kV, dtype=dtype), (kI, kJ, kV)


def _csr_coo(rp, ci, v):
    return np.repeat(np.arange(len(rp) - 1, dtype=np.int32), np.diff(rp)), np.asarray(ci, np.int32), np.asarray(v)


# ---- equality with selectref + from_coo ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", sorted(CASES))
def test_every_op_every_case(pkg, ctx, name, dtype):
    rows, cols, I, J, V, _ = CASES[name]
    Vd = _with_specials(CASES[name]).astype(dtype)
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, Vd, dtype=dtype)
    coo = _canonical(I, J, Vd, cols)
    for op in sel.OPS:
        for thunk in THUNKS[op]:
            R = A.select(op, thunk)
            want, _ = _expect(pkg, ctx, rows, cols, *coo, op, thunk, dtype)
            _assert_same_tiling(R, want, f"{name} {op}:{thunk}")


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", ("rand_300", "rect_70x40_AAt", "rect_33x65_AAt", "ragged_37", "powerlaw_600", "dense_48"))
def test_transposed_tiling_is_filtered_as_its_matrix(pkg, ctx, name, dtype):
    """a tiling built with transpose = 1 represents M^T: select works on M^T's coordinates"""
    rows, cols, I, J, V, _ = CASES[name]
    Vd = _with_specials(CASES[name]).astype(dtype)
    T = pkg.Tiled.from_coo(ctx, rows, cols, I, J, Vd, True, dtype=dtype)
    assert (T.rows, T.cols) == (cols, rows)
    coo = _canonical(J, I, Vd, rows)
    for op in sel.OPS:
        for thunk in THUNKS[op]:
            R = T.select(op, thunk)
            want, _ = _expect(pkg, ctx, cols, rows, *coo, op, thunk, dtype)
            _assert_same_tiling(R, want, f"{name}^T {op}:{thunk}")


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_value_thunks_nan_inf_and_rounding(pkg, ctx, dtype):
    rows = cols = 40
    rng = np.random.default_rng(9)
    key = np.sort(rng.choice(rows * cols, 600, replace=False))
    I, J = (key // cols).astype(np.int32), (key % cols).astype(np.int32)
    V = rng.choice(np.concatenate([SPECIAL, [0.1, -0.1, 1e-300, np.float32(0.1)]]), len(key)).astype(dtype)
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=dtype)
    for op in sel.OPS[8:]:
        for thunk in (np.nan, np.inf, -np.inf, -0.0, 0.1, 1e-40, 1e-300, 3.0e-310):
            want, _ = _expect(pkg, ctx, rows, cols, I, J, V, op, thunk, dtype)
            _assert_same_tiling(A.select(op, thunk), want, f"{op}:{thunk}")


def test_positional_thunks_at_the_limits(pkg, ctx):
    rows, cols, I, J, V, _ = CASES["band_1500"]
    I, J, V = _canonical(I, J, V, cols)
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    for op in sel.POSITIONAL:
        for k in (2 ** 31, -(2 ** 31), 1499, -1499, 1500, 17, -16, 15, 16, -17):
            want, _ = _expect(pkg, ctx, rows, cols, I, J, V, op, k, np.float64)
            _assert_same_tiling(A.select(op, k), want, f"{op}:{k}")


# ---- everything, nothing, empty operands -----------------------------------------------------------------------------------------
def test_everything_or_nothing_and_empty_result_as_operand(pkg, oracle, ctx):
    rows, cols, I, J, V, _ = CASES["powerlaw_600"]
    I, J, V = _canonical(I, J, V, cols)
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    for op, k in (("tril", 10 ** 6), ("triu", -(10 ** 6)), ("row_le", 599), ("col_gt", -1), ("value_le", np.inf), ("abs_gt", -1.0)):
        _assert_same_tiling(A.select(op, k), A, f"all {op}:{k}")
    for op, k in (("tril", -(10 ** 6)), ("triu", 10 ** 6), ("diag", 600), ("row_gt", 599), ("col_le", -1), ("value_gt", np.inf),
                  ("value_eq", np.nan), ("abs_gt", np.inf)):
        X = A.select(op, k)
        assert X.nnz == 0 and X.ntiles == 0 and (X.rows, X.cols) == (rows, cols), (op, k)
    rp, ci, v = X.export_csr()
    assert np.array_equal(rp, np.zeros(rows + 1, np.int32)) and len(ci) == len(v) == 0
    for P, Q in ((X, A), (A, X), (X, X)):
        p = pkg.CPlan(ctx, P, Q)
        p.spgemm()
        assert p.info()["nnz_c"] == 0
    pm = pkg.CPlan(ctx, A, A, mask=X)
    pm.spgemm()
    assert pm.info()["nnz_c"] == 0
    _assert_same_tiling(pkg.Tiled.ewise(X, A), A, "empty (+) A")
    Y = X.select("tril", 0)
    assert Y.nnz == 0 and Y.ntiles == 0
    Y.set_values_from_select(X)                             # the refresh of an empty result is a no-op
    E = pkg.Tiled.from_coo(ctx, 40, 40, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    for op in ("triu", "value_ne"):
        Z = E.select(op, 0)
        assert Z.nnz == 0 and Z.ntiles == 0 and (Z.rows, Z.cols) == (40, 40)


def test_select_of_select(pkg, ctx):
    rows, cols, I, J, V, _ = CASES["band_1500"]
    Vd = _with_specials(CASES["band_1500"])
    I, J, Vd = _canonical(I, J, Vd, cols)
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, Vd)
    R = A.select("tril", 5).select("value_ne", 0.0).select("abs_gt", 0.25).select("triu", -40)
    s = sel.select(I, J, Vd, "tril", 5)
    s = sel.select(*s, "value_ne", 0.0)
    s = sel.select(*s, "abs_gt", 0.25)
    s = sel.select(*s, "triu", -40)
    _assert_same_tiling(R, pkg.Tiled.from_coo(ctx, rows, cols, *s), "four selects")


# ---- a selected tiling as A, B and mask of a plan -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", ("rand_300", "powerlaw_600", "band_1500", "cancel_and_zero"))
def test_selected_as_operand_and_mask(pkg, oracle, ctx, name, dtype):
    rows, cols, I, J, V, _ = CASES[name]
    f32 = dtype == np.float32
    I, J, V = _canonical(I, J, np.asarray(V, dtype), cols)
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=dtype)
    Vq = V.astype(np.float64)
    oa = oracle.Csr(rows, cols, I, J, Vq)
    for op, k in (("tril", 0), ("abs_gt", 0.5), ("value_lt", 0.0), ("offdiag", 1)):
        R = A.select(op, k)
        s = sel.select(I, J, V, op, k, dtype)
        orr = oracle.Csr(rows, cols, s[0], s[1], s[2].astype(np.float64))
        for X, Y, ox, oy in ((R, A, orr, oa), (A, R, oa, orr), (R, R, orr, orr)):
            p = pkg.CPlan(ctx, X, Y)
            p.spgemm()
            got, want = p.export_csr(), oracle.csr_spgemm(ox, oy, f32=f32).arrays()
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), f"{name} {op}: structure"
            assert _same_vals(got[2], np.asarray(want[2]).astype(dtype)), f"{name} {op}: values"
        # R as a structural mask of A*A: the entries of the full product at R's positions
        pm = pkg.CPlan(ctx, A, A, mask=R)
        pm.spgemm()
        full = oracle.csr_spgemm(oa, oa, f32=f32).arrays()
        fI, fJ, fV = _csr_coo(*full)
        inR = np.isin(fI.astype(np.int64) * cols + fJ, s[0].astype(np.int64) * cols + s[1])
        mr, mc, mv = pm.export_csr()
        assert np.array_equal(np.diff(mr), np.bincount(fI[inR], minlength=rows)) and np.array_equal(mc, fJ[inR])
        assert _same_vals(mv, np.asarray(fV[inR]).astype(dtype))


# ---- graph workflows ---------------------------------------------------------------------------------------------------------
def _graph(seed, n, m):
    """an undirected simple graph: symmetric pattern, no self loops (values 1)"""
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, n, m), rng.integers(0, n, m)
    keep = a != b
    key = np.unique(np.concatenate([a[keep] * n + b[keep], b[keep] * n + a[keep]]))
    return (key // n).astype(np.int32), (key % n).astype(np.int32)


@pytest.mark.parametrize("n,m", ((120, 900), (400, 5000), (1000, 4000)))
def test_triangle_count_through_tril(pkg, ctx, n, m):
    """L = tril(A, -1); C<L> = L*L under plus_pair; sum(C) = triangles"""
    I, J = _graph(n + m, n, m)
    A = pkg.Tiled.from_coo(ctx, n, n, I, J, np.ones(len(I)))
    L = A.select("tril", -1)
    plan = pkg.CPlan(ctx, L, L, mask=L, semiring="plus_pair")
    plan.spgemm()
    got = int(plan.export_csr()[2].sum())
    D = np.zeros((n, n))
    D[I, J] = 1.0
    want = int(round(np.trace(D @ D @ D))) // 6
    assert got == want


def _truss_brute(n, I, J, k):
    E = set(zip(I.tolist(), J.tolist()))
    while True:
        nb = {}
        for u, v in E:
            nb.setdefault(u, set()).add(v)
        keep = {(u, v) for u, v in E if len(nb[u] & nb.get(v, set())) >= k - 2}
        if keep == E:
            return E
        E = keep


@pytest.mark.parametrize("k", (3, 4, 5))
def test_k_truss_peel(pkg, ctx, k):
    """repeat: support = C<A> = A*A under plus_pair; keep the edges with support >= k - 2; until nothing changes"""
    n = 300
    I, J = _graph(77, n, 2500)
    A = pkg.Tiled.from_coo(ctx, n, n, I, J, np.ones(len(I)))
    for _ in range(100):
        plan = pkg.CPlan(ctx, A, A, mask=A, semiring="plus_pair")
        plan.spgemm()
        S = pkg.Tiled.from_cplan(plan)
        A2 = S.select("value_ge", k - 2)
        done = A2.nnz == A.nnz
        A = A2
        if done:
            break
    rp, ci, _ = A.export_csr()
    got = set(zip(np.repeat(np.arange(n), np.diff(rp)).tolist(), ci.tolist()))
    assert got == _truss_brute(n, I, J, k)


# ---- positional refresh ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("transpose", (False, True), ids=("plain", "transposed"))
def test_refresh_equals_fresh(pkg, ctx, dtype, transpose):
    rows, cols, I, J, V, _ = CASES["powerlaw_600"]
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, np.asarray(V, dtype), transpose, dtype=dtype)
    rng = np.random.default_rng(41)
    for op, k in (("tril", -2), ("triu", 7), ("diag", 0), ("offdiag", 0), ("row_le", 300), ("row_gt", 17), ("col_le", 33), ("col_gt", 250)):
        R = A.select(op, k)
        down = pkg.CPlan(ctx, R, A)                          # a downstream plan on R (reads R's vals and A's vals_t)
        down.spgemm()
        for _ in range(2):
            A.set_values(rng.normal(size=A.nnz))
            R.set_values_from_select(A)
            ctx.synchronize()
            F = A.select(op, k)
            _assert_same_tiling(R, F, f"refresh {op}:{k}")
            down.step3()
            fresh = pkg.CPlan(ctx, F, A)
            fresh.spgemm()
            for x, y in zip(down.export_csr(), fresh.export_csr()):
                assert _same_vals(x, y) if x.dtype.kind == "f" else np.array_equal(x, y)
            # R as the B of a plan reads vals_t
            pb, pf = pkg.CPlan(ctx, A, R), pkg.CPlan(ctx, A, F)
            pb.spgemm()
            pf.spgemm()
            for x, y in zip(pb.export_csr(), pf.export_csr()):
                assert _same_vals(x, y) if x.dtype.kind == "f" else np.array_equal(x, y)


def test_refresh_refusals(pkg, ctx):
    rows, cols, I, J, V, _ = CASES["rand_300"]
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    R = A.select("tril", 0)
    for op in sel.OPS[8:]:
        Rv = A.select(op, 0.0)
        with pytest.raises(pkg.PemError) as e:
            Rv.set_values_from_select(A)                     # a value op: its pattern depends on the values
        assert e.value.status == PEM_E_INVALID and "select again" in str(e.value)
    A2 = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)         # same matrix, another tiling
    with pytest.raises(pkg.PemError) as e:
        R.set_values_from_select(A2)
    assert e.value.status == PEM_E_INVALID
    with pytest.raises(pkg.PemError) as e:
        A.set_values_from_select(R)                          # swapped arguments
    assert e.value.status == PEM_E_INVALID
    RR = R.select("triu", -3)
    with pytest.raises(pkg.PemError):
        RR.set_values_from_select(A)                         # made from R, not from A
    RR.set_values_from_select(R)
    R.set_values_from_select(A)                              # the right source
    ctx.synchronize()
    A.close()                                                # a tiling recreated (possibly at the same address)
    A3 = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    with pytest.raises(pkg.PemError):
        R.set_values_from_select(A3)


# ---- errors ---------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments(pkg, ctx):
    L = pkg.lib()
    rows, cols, I, J, V, _ = CASES["rand_50"]
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    h = C.c_void_p()

    def call(a, op, thunk, out=True, c=ctx._h):
        return L.pem_tiled_select(c, a, op, C.c_double(thunk), C.byref(h) if out else None)

    for op in (15, -1, 100):
        assert call(A._h, op, 0.0) == PEM_E_INVALID
    for op in range(8):
        for k in (0.5, -1.5, np.nan, np.inf, -np.inf, 2.0 ** 31 + 1, -(2.0 ** 31) - 1):
            assert call(A._h, op, k) == PEM_E_INVALID, (op, k)
    assert call(None, 0, 0.0) == PEM_E_INVALID
    assert call(A._h, 0, 0.0, out=False) == PEM_E_INVALID
    assert call(A._h, 0, 0.0, c=None) == PEM_E_INVALID
    assert L.pem_tiled_set_values_from_select(None, A._h, A._h) == PEM_E_INVALID
    assert L.pem_tiled_set_values_from_select(ctx._h, None, A._h) == PEM_E_INVALID
    R = A.select("tril", 0)
    assert L.pem_tiled_set_values_from_select(ctx._h, R._h, None) == PEM_E_INVALID
    assert call(A._h, 8, 0.5) == 0                            # (a value op takes any thunk)
    pkg.Tiled(ctx, h).close()
    with pytest.raises(ValueError):
        A.select("lower")
    with pytest.raises(pkg.PemError):
        A.select("tril", 0.5)


def test_result_save_load_and_info(pkg, ctx, tmp_path):
    rows, cols, I, J, V, _ = CASES["powerlaw_600"]
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    R = A.select("abs_gt", 0.5)
    assert R.conv_ms > 0
    path = str(tmp_path / "r.pemtile")
    R.save(path)
    _assert_same_tiling(pkg.Tiled.load(ctx, path), R, "save / load")
    assert pkg.flop_count(ctx, R, R) > 0
