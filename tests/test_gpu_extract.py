"""GPU: extract (pem_tiled_extract / pem_tiled_extract_device), transpose (pem_tiled_transpose) and their refreshes.

The central check: the tiling made on the device equals, array for array, the tiling pem_tiled_from_coo builds from extractref's COO of
the same matrix -- every pem_tiled_info field but the timings, all twelve arrays, values bit for bit.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import extractref as ex
from matgen import cases

pytestmark = pytest.mark.gpu

torch.cuda.is_available()   # (torch's runtime first, as in the other GPU files)

CASES = cases()
PEM_E_INVALID, PEM_E_OVERFLOW = -1, -4
DTYPES = (np.float64, np.float32)
INFO = ("rows", "cols", "nnz", "tile_rows", "tile_cols", "ntiles", "value_bytes")
ARRAYS = ("tile_keys", "tile_nnz_ptr", "masks", "rowptr", "rowcolidx", "vals", "masks_t", "tile_rowptr", "tile_colidx", "tile_colptr",
          "tile_rowidx", "tile_offsets")
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3.0e-310, 1.0e-40, 0.5, -0.5])
GIANT = 20000   # dimensions above this take ranges and sampled lists, not full permutations
KINDS = ("none", "aligned", "unaligned", "reversed", "perm", "repeats", "subset", "one_x40", "empty_only")


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32) if a.dtype.kind == "f" else a


def _same_vals(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and bool(np.all(_bits(got) == _bits(want)))


def _assert_same_tiling(got, want, label):
    for k in INFO:
        assert getattr(got, k) == getattr(want, k), f"{label}: {k} {getattr(got, k)} != {getattr(want, k)}"
    for name in ARRAYS:
        g, w = got.array(name), want.array(name)
        if name == "vals":
            assert _same_vals(g, w), f"{label}: vals differ"
        else:
            assert np.array_equal(g, w), f"{label}: array {name} differs"


def _same(x, y):
    return _same_vals(x, y) if np.asarray(x).dtype.kind == "f" else np.array_equal(x, y)


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


def _index_sets(rng, dim, used):
    """the index sets of the central check for a dimension of `dim` whose indices `used` hold entries; a giant dimension takes ranges
    and sampled lists in place of full-length ones"""
    giant = dim > GIANT
    n = min(dim, 3000) if giant else dim
    a0 = min(16 * ((dim // 4) // 16), max(dim - 1, 0))
    a1 = max(a0 + 1, min(dim, a0 + 16 * max(1, (n // 2) // 16)))
    u0 = min(3, dim - 1)
    u1 = max(u0 + 1, (u0 + n - 5) if giant else dim - 2)
    out = {"none": None, "aligned": np.arange(a0, a1), "unaligned": np.arange(u0, u1),
           "reversed": np.arange(dim - n, dim)[::-1], "perm": rng.permutation(dim) if not giant else rng.choice(dim, n, replace=False),
           "repeats": rng.integers(0, dim, n + n // 3 + 5), "subset": np.sort(rng.choice(dim, max(1, n // 3), replace=False)),
           "one_x40": np.full(40, int(rng.integers(0, dim)))}
    empty = np.setdiff1d(np.arange(dim), used)
    if len(empty):
        out["empty_only"] = empty[rng.permutation(len(empty))[:200]]
    return out


def _dev(L):
    return None if L is None else torch.as_tensor(np.ascontiguousarray(L, np.int32), device="cuda")


def _mxv(c, T, x, transpose):
    y = T.mxv(x, transpose=transpose)
    c.synchronize()                                       # (mxv never waits; the context may run on a stream of its own)
    return y.cpu().numpy()


def _want(pkg, ctx, rows, cols, coo, RI, CJ, dtype):
    ni, nj, oi, oj, ov = ex.extract(rows, cols, *coo, RI, CJ)
    return pkg.Tiled.from_coo(ctx, ni, nj, oi, oj, ov, dtype=dtype)


# ---- equality with extractref + from_coo -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", sorted(CASES))
def test_every_index_set_every_case(pkg, ctx, name, dtype):
    rows, cols, I, J, V, _ = CASES[name]
    Vd = _with_specials(CASES[name]).astype(dtype)
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, Vd, dtype=dtype)
    coo = _canonical(I, J, Vd, cols)
    rng = np.random.default_rng(rows * 31 + cols)
    rs, cs = _index_sets(rng, rows, I), _index_sets(rng, cols, J)
    for kind in KINDS:
        for RI, CJ, mode in ((rs.get(kind), None, "rows"), (None, cs.get(kind), "cols"), (rs.get(kind), cs.get(kind), "both")):
            if (mode != "cols" and kind not in rs) or (mode != "rows" and kind not in cs):
                continue                                  # (no empty row / column in this case)
            label = f"{name} {kind} {mode}"
            want = _want(pkg, ctx, rows, cols, coo, RI, CJ, dtype)
            _assert_same_tiling(A.extract(RI, CJ), want, label + " host")
            if kind != "none":
                _assert_same_tiling(A.extract(_dev(RI), _dev(CJ)), want, label + " device")
    # one list on the device, the other on the host; a slice
    RI, CJ = rs["repeats"], cs["subset"]
    want = _want(pkg, ctx, rows, cols, coo, RI, CJ, dtype)
    _assert_same_tiling(A.extract(_dev(RI), CJ), want, f"{name} device rows, host cols")
    _assert_same_tiling(A.extract(list(RI), _dev(CJ)), want, f"{name} host rows, device cols")
    sl = slice(1, None, 2) if rows > 1 else slice(None)
    _assert_same_tiling(A.extract(sl), _want(pkg, ctx, rows, cols, coo, np.arange(rows)[sl], None, dtype), f"{name} slice")


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", sorted(CASES))
def test_transpose_every_case(pkg, ctx, name, dtype):
    rows, cols, I, J, V, _ = CASES[name]
    Vd = _with_specials(CASES[name]).astype(dtype)
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, Vd, dtype=dtype)
    T = A.transpose()
    assert (T.rows, T.cols) == (cols, rows)
    _assert_same_tiling(T, pkg.Tiled.from_coo(ctx, rows, cols, I, J, Vd, True, dtype=dtype), f"{name}^T")
    rp, ci, v = A.export_csr()                            # ... also from A's exported entries
    ei = np.repeat(np.arange(rows, dtype=np.int32), np.diff(rp))
    _assert_same_tiling(T, pkg.Tiled.from_coo(ctx, rows, cols, ei, ci, v, True, dtype=dtype), f"{name}^T of the export")
    _assert_same_tiling(T.transpose(), A, f"({name}^T)^T")


# ---- round trips -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", ("rand_300", "rect_70x40_AAt", "powerlaw_600", "hub_row_4000", "band_1500", "one_entry", "row_vector_AAt"))
def test_permutation_and_its_inverse(pkg, ctx, name, dtype):
    rows, cols, I, J, V, _ = CASES[name]
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, _with_specials(CASES[name]).astype(dtype), dtype=dtype)
    rng = np.random.default_rng(12)
    p, q = rng.permutation(rows), rng.permutation(cols)
    R = A.extract(p, q)
    _assert_same_tiling(R.extract(np.argsort(p), np.argsort(q)), A, f"{name} p, q then their inverses")
    _assert_same_tiling(R.extract(_dev(np.argsort(p))).extract(None, np.argsort(q)), A, f"{name} inverses one side at a time")


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", ("rand_300", "rect_70x40_AAt", "band_1500", "blockrows_1600"))
def test_cplan_transposed_equals_transpose_of_cplan(pkg, ctx, name, dtype):
    rows, cols, I, J, V, tr = CASES[name]
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, np.asarray(V, dtype), dtype=dtype)
    B = pkg.Tiled.from_coo(ctx, rows, cols, I, J, np.asarray(V, dtype), True, dtype=dtype) if tr else A
    plan = pkg.CPlan(ctx, A, B)
    plan.spgemm()
    _assert_same_tiling(pkg.Tiled.from_cplan(plan).transpose(), pkg.Tiled.from_cplan(plan, transpose=True), f"{name}: C^T")


# ---- the device route a user had before: P*A*Q with selection matrices ----------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", ("rand_300", "rect_33x65_AAt", "powerlaw_600", "hub_row_4000", "empty_rows", "dense_48"))
def test_equals_the_products_with_selection_matrices(pkg, ctx, name, dtype):
    rows, cols, I, J, V, _ = CASES[name]
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, np.asarray(V, dtype), dtype=dtype)   # (no specials: 1 * a + 0 must be a)
    rng = np.random.default_rng(rows + 5)
    for RI, CJ in ((rng.permutation(rows), rng.permutation(cols)), (rng.integers(0, rows, rows + 20), rng.integers(0, cols, cols // 2 + 1)),
                   (np.full(17, rows - 1), np.arange(cols)[::-1])):
        pr, pc, pi, pj, pv = ex.selection(len(RI), rows, RI, left=True)
        qr, qc, qi, qj, qv = ex.selection(len(CJ), cols, CJ, left=False)
        P = pkg.Tiled.from_coo(ctx, pr, pc, pi, pj, pv, dtype=dtype)
        Q = pkg.Tiled.from_coo(ctx, qr, qc, qi, qj, qv, dtype=dtype)
        p1 = pkg.CPlan(ctx, P, A)
        p1.spgemm()
        p2 = pkg.CPlan(ctx, pkg.Tiled.from_cplan(p1), Q)
        p2.spgemm()
        _assert_same_tiling(A.extract(RI, CJ), pkg.Tiled.from_cplan(p2), f"{name}: P*A*Q")


# ---- input kinds -----------------------------------------------------------------------------------------------------------------
def _coo_of(T):
    rp, ci, v = T.export_csr()
    return np.repeat(np.arange(T.rows, dtype=np.int32), np.diff(rp)), np.asarray(ci, np.int32), np.asarray(v)


def _check_against_export(pkg, ctx, T, label, seed=0):
    """extract and transpose of any tiling T against extractref of T's exported entries"""
    rng = np.random.default_rng(seed + T.rows)
    coo = _coo_of(T)
    RI, CJ = rng.integers(0, T.rows, T.rows + 9), rng.permutation(T.cols)
    dtype = T.dtype.type
    _assert_same_tiling(T.extract(RI, CJ), _want(pkg, ctx, T.rows, T.cols, coo, RI, CJ, dtype), label + " extract")
    _assert_same_tiling(T.extract(_dev(RI)), _want(pkg, ctx, T.rows, T.cols, coo, RI, None, dtype), label + " extract rows (device)")
    tr, tc, ti, tj, tv = ex.transpose(T.rows, T.cols, *coo)
    _assert_same_tiling(T.transpose(), pkg.Tiled.from_coo(ctx, tr, tc, ti, tj, tv, dtype=dtype), label + " transpose")


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_every_kind_of_tiling_as_input(pkg, ctx, dtype, tmp_path):
    rows, cols, I, J, V, _ = CASES["powerlaw_600"]
    Vd = _with_specials(CASES["powerlaw_600"]).astype(dtype)
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, Vd, dtype=dtype)
    At = pkg.Tiled.from_coo(ctx, rows, cols, I, J, Vd, True, dtype=dtype)          # built with transpose = 1: its own matrix
    _check_against_export(pkg, ctx, At, "transpose=1")
    rr, rc, rI, rJ, rV, _ = CASES["rect_70x40_AAt"]
    Rt = pkg.Tiled.from_coo(ctx, rr, rc, rI, rJ, np.asarray(rV, dtype), True, dtype=dtype)
    assert (Rt.rows, Rt.cols) == (rc, rr)
    _check_against_export(pkg, ctx, Rt, "rect transpose=1")
    path = str(tmp_path / "a.pemtile")
    A.save(path)
    _check_against_export(pkg, ctx, pkg.Tiled.load(ctx, path), "loaded")
    _check_against_export(pkg, ctx, pkg.Tiled.ewise(A, At, "plus"), "ewise")
    _check_against_export(pkg, ctx, A.select("tril", 3), "select")
    _check_against_export(pkg, ctx, A.select("abs_gt", 0.5), "select by value")
    F = pkg.Tiled.from_coo(ctx, rows, cols, I, J, np.asarray(V, dtype), dtype=dtype)
    plan = pkg.CPlan(ctx, F, F)
    plan.spgemm()
    _check_against_export(pkg, ctx, pkg.Tiled.from_cplan(plan), "from_cplan")
    _check_against_export(pkg, ctx, pkg.Tiled.from_cplan(plan, transpose=True), "from_cplan transposed")
    X = torch.as_tensor(np.random.default_rng(1).normal(size=(rows, 3)).astype(dtype), device="cuda")
    _check_against_export(pkg, ctx, F.sddmm(X), "sddmm")
    _check_against_export(pkg, ctx, A.extract(np.arange(5, 500), None), "extract")
    _check_against_export(pkg, ctx, A.transpose(), "transpose")


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", ("rand_300", "powerlaw_600", "band_1500"))
def test_result_as_operand_and_mask(pkg, oracle, ctx, name, dtype):
    rows, cols, I, J, V, _ = CASES[name]
    f32 = dtype == np.float32
    I, J, V = _canonical(I, J, np.asarray(V, dtype), cols)
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=dtype)
    oa = oracle.Csr(rows, cols, I, J, V.astype(np.float64))
    rng = np.random.default_rng(rows)
    for RI, CJ in ((rng.permutation(rows), rng.permutation(cols)), (rng.integers(0, rows, rows), rng.integers(0, cols, cols))):
        for R, s in ((A.extract(RI, CJ), ex.extract(rows, cols, I, J, V, RI, CJ)), (A.transpose(), ex.transpose(rows, cols, I, J, V))):
            orr = oracle.Csr(rows, cols, s[2], s[3], s[4].astype(np.float64))
            for X, Y, ox, oy in ((R, A, orr, oa), (A, R, oa, orr), (R, R, orr, orr)):
                p = pkg.CPlan(ctx, X, Y)
                p.spgemm()
                got, want = p.export_csr(), oracle.csr_spgemm(ox, oy, f32=f32).arrays()
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), f"{name}: structure"
                assert _same_vals(got[2], np.asarray(want[2]).astype(dtype)), f"{name}: values"
            # R as a structural mask of A*A: the entries of the full product at R's positions
            pm = pkg.CPlan(ctx, A, A, mask=R)
            pm.spgemm()
            fr, fc, fv = (np.asarray(x) for x in oracle.csr_spgemm(oa, oa, f32=f32).arrays())
            fI = np.repeat(np.arange(rows, dtype=np.int32), np.diff(fr))
            inR = np.isin(fI.astype(np.int64) * cols + fc, s[2].astype(np.int64) * cols + s[3])
            mr, mc, mv = pm.export_csr()
            assert np.array_equal(np.diff(mr), np.bincount(fI[inR], minlength=rows)) and np.array_equal(mc, np.asarray(fc)[inR])
            assert _same_vals(mv, np.asarray(fv)[inR].astype(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_result_through_save_load_select_and_mxv(pkg, ctx, dtype, tmp_path):
    rows, cols, I, J, V, _ = CASES["rect_70x40_AAt"]
    I, J, V = _canonical(I, J, np.asarray(V, dtype), cols)
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=dtype)
    rng = np.random.default_rng(4)
    RI, CJ = rng.integers(0, rows, 100), rng.integers(0, cols, 55)
    for R, s in ((A.extract(RI, CJ), ex.extract(rows, cols, I, J, V, RI, CJ)), (A.transpose(), ex.transpose(rows, cols, I, J, V))):
        F = pkg.Tiled.from_coo(ctx, s[0], s[1], s[2], s[3], s[4], dtype=dtype)
        assert R.conv_ms > 0
        path = str(tmp_path / "r.pemtile")
        R.save(path)
        _assert_same_tiling(pkg.Tiled.load(ctx, path), R, "save / load")
        _assert_same_tiling(R.select("triu", -2), F.select("triu", -2), "select of the result")
        for tr in (False, True):
            x = torch.as_tensor(rng.normal(size=R.rows if tr else R.cols).astype(dtype), device="cuda")
            assert _same_vals(_mxv(ctx, R, x, tr), _mxv(ctx, F, x, tr)), f"mxv transpose={tr}"
        for x, y in zip(R.export_csr(), F.export_csr()):
            assert _same(x, y)
        assert pkg.flop_count(ctx, R, R.transpose()) == pkg.flop_count(ctx, F, F.transpose())


def test_empty_operands_and_results(pkg, ctx):
    E = pkg.Tiled.from_coo(ctx, 40, 30, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    for R, shape in ((E.extract([3, 3, 1], None), (3, 30)), (E.extract(None, [0]), (40, 1)), (E.extract([39], [29, 0]), (1, 2)), (E.transpose(), (30, 40)),
                     (E.extract(), (40, 30))):
        assert (R.rows, R.cols) == shape and R.nnz == 0 and R.ntiles == 0
        rp, ci, v = R.export_csr()
        assert np.array_equal(rp, np.zeros(shape[0] + 1, np.int32)) and len(ci) == len(v) == 0
    R = E.extract([1, 2], None)
    R.set_values_from_extract(E)                          # the refresh of an empty result is a no-op
    T = E.transpose()
    T.set_values_from_transpose(E)
    rows, cols, I, J, V, _ = CASES["empty_rows"]
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    empty = np.setdiff1d(np.arange(rows), I)
    X = A.extract(empty, None)
    assert X.nnz == 0 and X.ntiles == 0 and (X.rows, X.cols) == (len(empty), cols)
    p = pkg.CPlan(ctx, X, A)
    p.spgemm()
    assert p.info()["nnz_c"] == 0


# ---- refresh ---------------------------------------------------------------------------------------------------------------------
def _left(pkg, c, n, dtype):
    """a 24 x n operand for a plan whose B is an n-row tiling"""
    rng = np.random.default_rng(n)
    key = np.sort(rng.choice(24 * n, min(24 * n, 6 * n), replace=False))
    return pkg.Tiled.from_coo(c, 24, n, (key // n).astype(np.int32), (key % n).astype(np.int32), rng.normal(size=len(key)).astype(dtype), dtype=dtype)


def _refresh_rounds(pkg, c, ref_ctx, dtype, aged, rounds=3, name="powerlaw_600"):
    """set_values on A in row and in column order, then the refreshes, against fresh builds: vals array for array, vals_t through
    mxv(transpose=True) and through a plan's B side"""
    rows, cols, I, J, V, _ = CASES[name]
    A = pkg.Tiled.from_coo(c, rows, cols, I, J, np.asarray(V, dtype), dtype=dtype)
    rng = np.random.default_rng(41)
    RI, CJ = rng.integers(0, rows, rows + 30), rng.permutation(cols)[: cols - 7]
    made = {"extract": lambda X: X.extract(RI, CJ), "extract rows": lambda X: X.extract(_dev(RI)), "extract cols": lambda X: X.extract(None, CJ),
            "transpose": lambda X: X.transpose()}
    R = {k: f(A) for k, f in made.items()}
    x = {k: torch.as_tensor(rng.normal(size=t.rows).astype(dtype), device="cuda") for k, t in R.items()}
    torch.cuda.synchronize()
    if aged:                                              # handles that already hold vmap_t and the column schedule
        for k, t in R.items():
            t.mxv(x[k], transpose=True)
            t.set_values(rng.normal(size=t.nnz))
    down = {k: pkg.CPlan(c, _left(pkg, c, t.rows, dtype), t) for k, t in R.items()}   # R as B: step 3 reads vals_t
    for p in down.values():
        p.spgemm()
    ci = _canonical(I, J, np.arange(len(I)), cols)[:2]
    for rnd in range(rounds):
        V2 = rng.normal(size=A.nnz)
        if rnd % 2 == 0:
            A.set_values(V2, "row")
            Vfull = V2
        else:
            A.set_values(V2, "col")                       # V2 ordered by (col, row): back to row order for the fresh build
            o = np.argsort(ci[1].astype(np.int64) * rows + ci[0], kind="stable")
            Vfull = np.empty_like(V2)
            Vfull[o] = V2
        Fa = pkg.Tiled.from_coo(ref_ctx, rows, cols, ci[0], ci[1], Vfull.astype(dtype), dtype=dtype)
        for k, t in R.items():
            if k == "transpose":
                t.set_values_from_transpose(A)
            else:
                t.set_values_from_extract(A)
            c.synchronize()
            F = made[k](Fa)
            _assert_same_tiling(t, F, f"refresh {k} round {rnd}")
            assert _same_vals(_mxv(c, t, x[k], True), _mxv(ref_ctx, F, x[k], True)), f"{k}: vals_t by mxv"
            down[k].step3()
            fresh = pkg.CPlan(ref_ctx, _left(pkg, ref_ctx, F.rows, dtype), F)
            fresh.spgemm()
            for a, b in zip(down[k].export_csr(), fresh.export_csr()):
                assert _same(a, b), f"{k}: the B side of a plan"


@pytest.mark.parametrize("aged", (False, True), ids=("fresh", "aged"))
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_refresh_equals_fresh(pkg, ctx, dtype, aged):
    _refresh_rounds(pkg, ctx, ctx, dtype, aged)


def test_refresh_on_a_graph_replay_context(pkg, ctx):
    g = pkg.Context(0)
    try:
        g.set_graph_replay(True)
        rows, cols, I, J, V, _ = CASES["band_1500"]
        A = pkg.Tiled.from_coo(g, rows, cols, I, J, V)
        rng = np.random.default_rng(8)
        p = rng.permutation(rows)
        R, T = A.extract(p, p), A.transpose()
        pr, pt = pkg.CPlan(g, R, A), pkg.CPlan(g, A, T)
        for _ in range(3):
            pr.spgemm()                                   # captured, then replayed
            pt.spgemm()
        ci = _canonical(I, J, np.arange(len(I)), cols)
        for seed in (21, 22, 23):
            V2 = np.random.default_rng(seed).normal(size=A.nnz)
            A.set_values(V2)
            R.set_values_from_extract(A)
            T.set_values_from_transpose(A)
            pr.spgemm()
            pt.spgemm()
            A2 = pkg.Tiled.from_coo(ctx, rows, cols, ci[0], ci[1], V2)
            fr, ft = pkg.CPlan(ctx, A2.extract(p, p), A2), pkg.CPlan(ctx, A2, A2.transpose())
            fr.spgemm()
            ft.spgemm()
            for got, want in ((pr, fr), (pt, ft)):
                for x, y in zip(got.export_csr(), want.export_csr()):
                    assert _same(x, y), seed
    finally:
        g.close()


def test_refresh_on_a_stream_context(pkg, ctx):
    prev = torch.cuda.current_stream()
    stream = torch.cuda.Stream()                          # (not the null stream: the context would make its own)
    g = pkg.Context(0, stream=stream.cuda_stream)
    try:
        torch.cuda.set_stream(stream)
        _refresh_rounds(pkg, g, ctx, np.float64, aged=True, rounds=3, name="rand_300")
    finally:
        torch.cuda.set_stream(prev)
        g.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def _snapshot(T):
    return {n: T.array(n).copy() for n in ARRAYS}


def _unchanged(pkg, T, snap, label):
    info = pkg.TiledInfo()
    assert pkg.lib().pem_tiled_get_info(T._h, C.byref(info)) == 0
    for k in INFO:
        assert getattr(info, k) == getattr(T, k), f"{label}: {k} changed"
    for n in ARRAYS:
        assert _same(T.array(n), snap[n]), f"{label}: array {n} changed"


def test_refusals_leave_every_handle_unchanged(pkg, ctx):
    L = pkg.lib()
    rows, cols, I, J, V, _ = CASES["rect_70x40_AAt"]
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    snap = _snapshot(A)
    h = C.c_void_p()

    def host(I_, ni, J_, nj, out=True, a=A._h, c=ctx._h):
        pi = None if I_ is None else np.ascontiguousarray(I_, np.int32)
        pj = None if J_ is None else np.ascontiguousarray(J_, np.int32)
        return L.pem_tiled_extract(c, a, None if pi is None else pi.ctypes.data_as(C.c_void_p), C.c_int64(ni),
                                   None if pj is None else pj.ctypes.data_as(C.c_void_p), C.c_int64(nj), C.byref(h) if out else None)

    def device(I_, ni, J_, nj, out=True):
        di, dj = _dev(I_), _dev(J_)
        torch.cuda.synchronize()
        return L.pem_tiled_extract_device(ctx._h, A._h, None if di is None else C.c_void_p(di.data_ptr()), C.c_int64(ni),
                                          None if dj is None else C.c_void_p(dj.data_ptr()), C.c_int64(nj), C.byref(h) if out else None)

    for fn in (host, device):
        for bad_i, bad_j in (([0, -1, 3], None), ([0, rows, 3], None), (None, [cols]), (None, [1, 2, -1]), ([5], [cols]), ([rows], [0]),
                             ([2 ** 31 - 1], None), ([-(2 ** 31)], None)):
            h.value = 12345
            st = fn(bad_i, 0 if bad_i is None else len(bad_i), bad_j, 0 if bad_j is None else len(bad_j))
            assert st == PEM_E_INVALID and h.value is None, (fn.__name__, bad_i, bad_j)
        for ni, nj in ((0, 1), (1, 0), (-3, 1), (2 ** 31, 1)):   # n < 1 or n > INT32_MAX with a non-null list
            h.value = 12345
            assert fn([0], ni, [0], nj) == PEM_E_INVALID and h.value is None, (fn.__name__, ni, nj)
        assert fn([0], 1, [0], 1, out=False) == PEM_E_INVALID
        _unchanged(pkg, A, snap, fn.__name__)
    assert host([0], 1, None, 0, a=None) == PEM_E_INVALID
    assert host([0], 1, None, 0, c=None) == PEM_E_INVALID
    assert L.pem_tiled_transpose(ctx._h, A._h, None) == PEM_E_INVALID
    assert L.pem_tiled_transpose(ctx._h, None, C.byref(h)) == PEM_E_INVALID
    assert L.pem_tiled_transpose(None, A._h, C.byref(h)) == PEM_E_INVALID
    for f in (L.pem_tiled_set_values_from_extract, L.pem_tiled_set_values_from_transpose):
        assert f(None, A._h, A._h) == PEM_E_INVALID and f(ctx._h, None, A._h) == PEM_E_INVALID and f(ctx._h, A._h, None) == PEM_E_INVALID
    assert host(None, 77, None, -5) == 0                  # null lists are "all": their counts are ignored
    _assert_same_tiling(pkg.Tiled(ctx, C.c_void_p(h.value)), A, "A(:, :)")
    # the Python layer: negative indices are refused, not wrapped; values must be integers
    for bad in ([-1], [rows], [0.5], [[0, 1]]):
        with pytest.raises(ValueError):
            A.extract(bad)
    with pytest.raises(ValueError):
        A.extract(None, torch.zeros(3, dtype=torch.int64, device="cuda"))
    with pytest.raises(pkg.PemError) as e:
        A.extract([])
    assert e.value.status == PEM_E_INVALID
    with pytest.raises(pkg.PemError) as e:
        A.extract(torch.tensor([0, rows], dtype=torch.int32, device="cuda"))
    assert e.value.status == PEM_E_INVALID
    _unchanged(pkg, A, snap, "python refusals")


def test_refresh_refusals(pkg, ctx):
    rows, cols, I, J, V, _ = CASES["rand_300"]
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    R, T, S = A.extract(np.arange(100), None), A.transpose(), A.select("tril", 0)
    snaps = {k: _snapshot(t) for k, t in (("R", R), ("T", T), ("S", S), ("A", A))}
    A2 = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)      # same matrix, another tiling
    for call in (lambda: R.set_values_from_extract(A2), lambda: T.set_values_from_transpose(A2),
                 lambda: S.set_values_from_extract(A), lambda: S.set_values_from_transpose(A),      # a select-made tiling
                 lambda: R.set_values_from_transpose(A), lambda: T.set_values_from_extract(A),      # the other builder's refresh
                 lambda: R.set_values_from_select(A), lambda: A.set_values_from_extract(R), lambda: A.set_values_from_transpose(T)):
        with pytest.raises(pkg.PemError) as e:
            call()
        assert e.value.status == PEM_E_INVALID
    RR, TT = R.extract(None, [5, 5, 2]), T.transpose()
    with pytest.raises(pkg.PemError):
        RR.set_values_from_extract(A)                     # made from R, not from A
    with pytest.raises(pkg.PemError):
        TT.set_values_from_transpose(A)
    for k, t in (("R", R), ("T", T), ("S", S), ("A", A)):
        _unchanged(pkg, t, snaps[k], k)
    RR.set_values_from_extract(R)
    TT.set_values_from_transpose(T)
    R.set_values_from_extract(A)                          # the right source
    T.set_values_from_transpose(A)
    ctx.synchronize()
    A.close()                                             # a tiling recreated (possibly at the same address)
    A3 = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    with pytest.raises(pkg.PemError):
        R.set_values_from_extract(A3)
    with pytest.raises(pkg.PemError):
        T.set_values_from_transpose(A3)


# ---- overflow, determinism ----------------------------------------------------------------------------------------------------
def test_overflow_is_found_before_the_payload_is_allocated(pkg, ctx):
    n = 65536
    A = pkg.Tiled.from_coo(ctx, 1, n, np.zeros(n, np.int32), np.arange(n, dtype=np.int32), np.ones(n))
    # the same list on a row with one entry per tile is within the range: it works, and the context's own scratch (the scans' block
    # sums, grow-only and counted in in_use_bytes) has then seen a call of this size
    S = pkg.Tiled.from_coo(ctx, 1, n, np.zeros(n // 16, np.int32), np.arange(0, n, 16, dtype=np.int32), np.ones(n // 16))
    ok = S.extract([0] * 32768)
    assert ok.nnz == 32768 * (n // 16) and ok.ntiles == 2048 * (n // 16)
    ok.close()
    At = A.transpose()
    ctx.synchronize()
    before = ctx.memory_stats()["in_use_bytes"]
    for L in ([0] * 32768, _dev(np.zeros(32768, np.int32))):   # 2^31 entries
        with pytest.raises(pkg.PemError) as e:
            A.extract(L)
        assert e.value.status == PEM_E_OVERFLOW and "int32" in str(e.value)
        assert ctx.memory_stats()["in_use_bytes"] == before
    with pytest.raises(pkg.PemError) as e:                # ... and through the column side
        At.extract(None, [0] * 32768)
    assert e.value.status == PEM_E_OVERFLOW
    assert ctx.memory_stats()["in_use_bytes"] == before
    _assert_same_tiling(A.extract([0]), A, "A still works")


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_two_calls_give_identical_bytes(pkg, ctx, dtype):
    rows, cols, I, J, V, _ = CASES["hub_row_4000"]
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, _with_specials(CASES["hub_row_4000"]).astype(dtype), dtype=dtype)
    rng = np.random.default_rng(6)
    RI, CJ = rng.integers(0, rows, 2 * rows), rng.integers(0, cols, cols)
    for make in (lambda: A.extract(RI, CJ), lambda: A.extract(_dev(RI), None), lambda: A.transpose()):
        X, Y = make(), make()
        for n in ARRAYS:
            assert X.array(n).tobytes() == Y.array(n).tobytes(), n
