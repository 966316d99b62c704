"""GPU: assign (pem_tiled_assign / pem_tiled_assign_device) and its refresh (pem_tiled_set_values_from_assign).

The central check: the tiling made on the device equals, array for array, the tiling pem_tiled_from_coo builds from assignref's COO of
the same matrices -- every pem_tiled_info field but the timings, all twelve arrays, values bit for bit (under an accum by
test_gpu_ewise's rule: NaN matches NaN, the sign of a zero is free under min / max).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import assignref as ar
import ewiseref as er
from matgen import cases
from test_gpu_ewise import _same_vals as _same_vals_op
from test_gpu_extract import ARRAYS, INFO, _assert_same_tiling, _canonical, _dev, _mxv, _same, _same_vals, _snapshot, _unchanged, _with_specials

pytestmark = pytest.mark.gpu

torch.cuda.is_available()   # (torch's runtime first, as in the other GPU files)

CASES = cases()
PEM_E_INVALID = -1
DTYPES = (np.float64, np.float32)
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3.0e-310, 1.0e-40, 0.5, -0.5])
EW_SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 2.0])   # test_gpu_ewise's
SMALL = ("tiny_9x9", "one_entry", "rand_50", "rand_300", "rect_70x40_AAt", "rect_33x65_AAt", "ragged_37", "dense_tile", "dense_48",
         "empty_rows", "empty_matrix", "row_vector_AAt", "col_vector_AAt", "powerlaw_600", "hub_row_4000", "band_1500")
KINDS = ("none", "aligned", "unaligned", "straddle", "last_tile", "reversed", "perm", "subset", "unsorted", "single")


def _index_sets(rng, dim, cap=None):
    """the list kinds of the central check for a dimension; cap: sample the long ones down to this many indices"""
    n = dim if cap is None else min(dim, cap)
    a0 = 16 * ((dim // 4) // 16)
    a1 = max(a0 + 1, min(dim, a0 + 16 * max(1, (n // 2) // 16)))
    u0 = min(3, dim - 1)
    u1 = max(u0 + 1, min(dim - 2, u0 + n - 5))
    some = rng.choice(dim, n, replace=False) if n < dim else rng.permutation(dim)
    return {"none": None, "aligned": np.arange(a0, a1), "unaligned": np.arange(u0, u1),
            "straddle": np.array([x for x in (15, 16) if x < dim] or [dim - 1]), "last_tile": np.arange(16 * ((dim - 1) // 16), dim),
            "reversed": np.arange(dim - n, dim)[::-1], "perm": some, "subset": np.sort(some[: max(1, n // 3)]),
            "unsorted": some[: max(1, n // 2)], "single": np.array([int(rng.integers(0, dim))])}


def _operand(rng, ni, nj, nnz, dtype, special=SPECIAL):
    """a canonical ni x nj COO of about nnz entries (all of them where nnz >= ni * nj), about a fifth of the values special"""
    if nnz >= ni * nj:
        key = np.arange(ni * nj, dtype=np.int64)
    else:
        key = np.unique(rng.integers(0, ni * nj, nnz))
    V = rng.normal(size=len(key))
    sp = rng.random(len(key)) < 0.2
    V[sp] = rng.choice(special, int(sp.sum()))
    return (key // nj).astype(np.int32), (key % nj).astype(np.int32), V.astype(dtype)


def _len(L, dim):
    return dim if L is None else len(L)


def _tiled(pkg, ctx, rows, cols, coo, dtype):
    return pkg.Tiled.from_coo(ctx, rows, cols, coo[0], coo[1], coo[2], dtype=dtype)


def _want(pkg, ctx, rows, cols, c, a, RI, CJ, accum, dtype):
    return _tiled(pkg, ctx, rows, cols, ar.assign(rows, cols, c, a, RI, CJ, accum), dtype)


def _assert_same_accum(got, want, label, op):
    for k in INFO:
        assert getattr(got, k) == getattr(want, k), f"{label}: {k} {getattr(got, k)} != {getattr(want, k)}"
    for name in ARRAYS:
        g, w = got.array(name), want.array(name)
        if name == "vals":
            assert _same_vals_op(g, w, op), f"{label}: vals differ"
        else:
            assert np.array_equal(g, w), f"{label}: array {name} differs"


def _coo_of(T):
    rp, ci, v = T.export_csr()
    return np.repeat(np.arange(T.rows, dtype=np.int32), np.diff(rp)), np.asarray(ci, np.int32), np.asarray(v)


def _empty(pkg, ctx, rows, cols, dtype):
    z = np.zeros(0, np.int32)
    return pkg.Tiled.from_coo(ctx, rows, cols, z, z, np.zeros(0, dtype), dtype=dtype)


# ---- 1. every index kind on the small cases, no accum -------------------------------------------------------------------------------
def _every_kind(pkg, ctx, name, dtype, cap=None):
    rows, cols, I, J, V, _ = CASES[name]
    Vd = _with_specials(CASES[name]).astype(dtype)
    Ct = pkg.Tiled.from_coo(ctx, rows, cols, I, J, Vd, dtype=dtype)
    c = _canonical(I, J, Vd, cols)
    snap = _snapshot(Ct)
    rng = np.random.default_rng(rows * 31 + cols)
    rs, cs = _index_sets(rng, rows, cap), _index_sets(rng, cols, cap)
    density = len(I) / (rows * cols)
    for kind in KINDS:
        for RI, CJ, mode in ((rs[kind], None, "rows"), (None, cs[kind], "cols"), (rs[kind], cs[kind], "both")):
            ni, nj = _len(RI, rows), _len(CJ, cols)
            fills = [("empty", 0), ("like C", max(1, int(density * ni * nj)))] + ([("full", ni * nj)] if ni * nj <= 4096 else [])
            for fname, nnz in fills:
                label = f"{name} {kind} {mode} {fname}"
                a = _operand(rng, ni, nj, nnz, dtype)
                At = _tiled(pkg, ctx, ni, nj, a, dtype)
                want = _want(pkg, ctx, rows, cols, c, a, RI, CJ, None, dtype)
                _assert_same_tiling(Ct.assign(At, RI, CJ), want, label + " host")
                if kind != "none" and fname == "like C":
                    _assert_same_tiling(Ct.assign(At, _dev(RI), _dev(CJ)), want, label + " device")
    # one list on the device, the other on the host; a slice
    RI, CJ = rs["unsorted"], cs["subset"]
    a = _operand(rng, len(RI), len(CJ), max(1, int(density * len(RI) * len(CJ))), dtype)
    At = _tiled(pkg, ctx, len(RI), len(CJ), a, dtype)
    want = _want(pkg, ctx, rows, cols, c, a, RI, CJ, None, dtype)
    _assert_same_tiling(Ct.assign(At, _dev(RI), CJ), want, f"{name} device rows, host cols")
    _assert_same_tiling(Ct.assign(At, list(RI), _dev(CJ)), want, f"{name} host rows, device cols")
    if cap is None:
        sl = slice(1, None, 2) if rows > 1 else slice(None)
        RI = np.arange(rows)[sl]
        a = _operand(rng, len(RI), cols, max(1, int(density * len(RI) * cols)), dtype)
        _assert_same_tiling(Ct.assign(_tiled(pkg, ctx, len(RI), cols, a, dtype), sl), _want(pkg, ctx, rows, cols, c, a, RI, None, None, dtype),
                            f"{name} slice")
    _unchanged(pkg, Ct, snap, f"{name}: C after the assigns")


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", SMALL)
def test_every_index_kind_every_case(pkg, ctx, name, dtype):
    _every_kind(pkg, ctx, name, dtype)


# ---- 2. 16 385 tile rows: a key-width boundary -----------------------------------------------------------------------------------------
def test_wide_tilecols(pkg, ctx):
    _every_kind(pkg, ctx, "wide_tilecols", np.float64, cap=3000)


# ---- 3. accum --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("op", er.OPS)
@pytest.mark.parametrize("name", ("rand_300", "rect_70x40_AAt"))
def test_accum(pkg, ctx, name, op, dtype):
    rows, cols, I, J, V, _ = CASES[name]
    rng = np.random.default_rng(rows + len(op))
    Vd = np.array(V, np.float64)
    sp = rng.random(len(Vd)) < 0.2
    Vd[sp] = rng.choice(EW_SPECIAL, int(sp.sum()))
    c = _canonical(I, J, Vd.astype(dtype), cols)
    Ct = _tiled(pkg, ctx, rows, cols, c, dtype)
    rs, cs = _index_sets(rng, rows), _index_sets(rng, cols)
    for kr, kc in (("unsorted", "subset"), ("perm", "perm"), ("aligned", "none"), ("none", "straddle"), ("none", "none")):
        RI, CJ = rs[kr], cs[kc]
        ni, nj = _len(RI, rows), _len(CJ, cols)
        # A: about half of C's entries in the region (at their source positions), plus as many elsewhere
        inv_r, inv_c = np.full(rows, -1), np.full(cols, -1)
        inv_r[np.arange(rows) if RI is None else RI] = np.arange(ni)
        inv_c[np.arange(cols) if CJ is None else CJ] = np.arange(nj)
        inside = np.flatnonzero((inv_r[c[0]] >= 0) & (inv_c[c[1]] >= 0))
        hit = inside[rng.random(len(inside)) < 0.5]
        key = np.unique(np.concatenate([inv_r[c[0][hit]].astype(np.int64) * nj + inv_c[c[1][hit]], rng.integers(0, ni * nj, len(hit) + 3)]))
        va = rng.normal(size=len(key))
        sp = rng.random(len(key)) < 0.2
        va[sp] = rng.choice(EW_SPECIAL, int(sp.sum()))
        a = ((key // nj).astype(np.int32), (key % nj).astype(np.int32), va.astype(dtype))
        At = _tiled(pkg, ctx, ni, nj, a, dtype)
        want = _want(pkg, ctx, rows, cols, c, a, RI, CJ, op, dtype)
        assert want.nnz < Ct.nnz + At.nnz or len(hit) == 0            # (some entries are fed by both)
        _assert_same_accum(Ct.assign(At, RI, CJ, accum=op), want, f"{name} {op} {kr} x {kc}", op)
        _assert_same_accum(Ct.assign(At, _dev(RI), _dev(CJ), accum=op), want, f"{name} {op} {kr} x {kc} device", op)
        if RI is None and CJ is None:
            _assert_same_accum(Ct.assign(At, accum=op), pkg.Tiled.ewise(Ct, At, op), f"{name} {op}: ewise", op)


# ---- 4. round trips and identities ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", ("rand_300", "rect_70x40_AAt", "powerlaw_600", "hub_row_4000"))
def test_round_trips_and_identities(pkg, ctx, name, dtype):
    rows, cols, I, J, V, _ = CASES[name]
    Vd = _with_specials(CASES[name]).astype(dtype)
    Ct = pkg.Tiled.from_coo(ctx, rows, cols, I, J, Vd, dtype=dtype)
    c = _canonical(I, J, Vd, cols)
    rng = np.random.default_rng(rows + 17)
    E = _empty(pkg, ctx, rows, cols, dtype)
    for p, q, full in ((rng.permutation(rows), rng.permutation(cols), True),
                       (rng.permutation(rows)[: rows // 3], np.sort(rng.permutation(cols)[: cols // 2]), False)):
        _assert_same_tiling(Ct.assign(Ct.extract(p, q), p, q), Ct, f"{name}: C(p, q) written back")
        a = _operand(rng, len(p), len(q), max(1, len(I) * len(p) * len(q) // (rows * cols)), dtype)
        At = _tiled(pkg, ctx, len(p), len(q), a, dtype)
        if full:
            _assert_same_tiling(E.assign(At, p, q), At.extract(np.argsort(p), np.argsort(q)), f"{name}: into an empty tiling")
        Z = Ct.assign(At, _dev(p), q)
        _assert_same_tiling(Z.extract(p, q), At, f"{name}: Z(I, J) is A")
        hole = _empty(pkg, ctx, len(p), len(q), dtype)
        _assert_same_tiling(Z.assign(hole, p, q), Ct.assign(hole, p, q), f"{name}: Z outside the region is C")
    # block assembly [A B; C D]: four assigns into an empty tiling
    r0, c0 = rows // 2 + 3, cols // 3 + 1
    blocks = []
    Z = E
    for (i0, i1), (j0, j1) in (((0, r0), (0, c0)), ((0, r0), (c0, cols)), ((r0, rows), (0, c0)), ((r0, rows), (c0, cols))):
        b = _operand(rng, i1 - i0, j1 - j0, max(1, len(I) * (i1 - i0) * (j1 - j0) // (rows * cols)), dtype)
        blocks.append((b[0] + i0, b[1] + j0, b[2]))
        Z = Z.assign(_tiled(pkg, ctx, i1 - i0, j1 - j0, b, dtype), slice(i0, i1), slice(j0, j1))
    s = _canonical(*(np.concatenate([b[k] for b in blocks]) for k in range(3)), cols)
    _assert_same_tiling(Z, _tiled(pkg, ctx, rows, cols, s, dtype), f"{name}: block assembly")


# ---- 5. every kind of tiling as C and as A -------------------------------------------------------------------------------------------
def _check_against_export(pkg, ctx, T, label):
    """T as C and as A of an assign, without and with an accum, against assignref of T's exported entries"""
    rng = np.random.default_rng(T.rows + 3)
    t = _coo_of(T)
    dtype = T.dtype.type
    RI, CJ = rng.permutation(T.rows)[: max(1, T.rows // 2)], rng.permutation(T.cols)[: max(1, 2 * T.cols // 3)]
    a = _operand(rng, len(RI), len(CJ), max(1, T.nnz * len(RI) * len(CJ) // (T.rows * T.cols)), dtype, EW_SPECIAL)
    At = _tiled(pkg, ctx, len(RI), len(CJ), a, dtype)
    _assert_same_tiling(T.assign(At, RI, CJ), _want(pkg, ctx, T.rows, T.cols, t, a, RI, CJ, None, dtype), label + " as C")
    _assert_same_accum(T.assign(At, _dev(RI), CJ, accum="plus"), _want(pkg, ctx, T.rows, T.cols, t, a, RI, CJ, "plus", dtype), label + " as C, plus",
                       "plus")
    rows, cols = T.rows + 21, T.cols + 5
    b = _operand(rng, rows, cols, max(1, T.nnz), dtype, EW_SPECIAL)
    Bt = _tiled(pkg, ctx, rows, cols, b, dtype)
    RI, CJ = rng.permutation(rows)[: T.rows], rng.permutation(cols)[: T.cols]
    _assert_same_tiling(Bt.assign(T, RI, _dev(CJ)), _want(pkg, ctx, rows, cols, b, t, RI, CJ, None, dtype), label + " as A")
    _assert_same_accum(Bt.assign(T, RI, CJ, accum="max"), _want(pkg, ctx, rows, cols, b, t, RI, CJ, "max", dtype), label + " as A, max", "max")


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_every_kind_of_tiling_as_c_and_as_a(pkg, ctx, dtype, tmp_path):
    rows, cols, I, J, V, _ = CASES["powerlaw_600"]
    Vd = np.asarray(V, dtype)
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, Vd, dtype=dtype)
    At = pkg.Tiled.from_coo(ctx, rows, cols, I, J, Vd, True, dtype=dtype)          # built with transpose = 1: its own matrix
    _check_against_export(pkg, ctx, At, "transpose=1")
    rr, rc, rI, rJ, rV, _ = CASES["rect_70x40_AAt"]
    Rt = pkg.Tiled.from_coo(ctx, rr, rc, rI, rJ, np.asarray(rV, dtype), True, dtype=dtype)
    _check_against_export(pkg, ctx, Rt, "rect transpose=1")
    path = str(tmp_path / "a.pemtile")
    A.save(path)
    _check_against_export(pkg, ctx, pkg.Tiled.load(ctx, path), "loaded")
    _check_against_export(pkg, ctx, pkg.Tiled.ewise(A, At, "plus"), "ewise")
    _check_against_export(pkg, ctx, A.select("tril", 3), "select")
    plan = pkg.CPlan(ctx, A, A)
    plan.spgemm()
    _check_against_export(pkg, ctx, pkg.Tiled.from_cplan(plan), "from_cplan")
    X = torch.as_tensor(np.random.default_rng(1).normal(size=(rows, 3)).astype(dtype), device="cuda")
    _check_against_export(pkg, ctx, A.sddmm(X), "sddmm")
    _check_against_export(pkg, ctx, A.extract(np.arange(5, 500), None), "extract")
    _check_against_export(pkg, ctx, A.transpose(), "transpose")
    _check_against_export(pkg, ctx, A.assign(A.extract(np.arange(40), np.arange(9, 90)), np.arange(100, 140), np.arange(81)), "assign")
    _assert_same_tiling(A.assign(A), A, "C and A the same handle")
    Z = A.assign(A, accum="plus")
    _assert_same_accum(Z, pkg.Tiled.ewise(A, A, "plus"), "C and A the same handle, plus", "plus")


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_result_as_operand_and_mask(pkg, oracle, ctx, dtype):
    rows, cols, I, J, V, _ = CASES["rand_300"]
    f32 = dtype == np.float32
    I, J, V = _canonical(I, J, np.asarray(V, dtype), cols)
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=dtype)
    oa = oracle.Csr(rows, cols, I, J, V.astype(np.float64))
    rng = np.random.default_rng(rows)
    RI, CJ = rng.permutation(rows)[:120], rng.permutation(cols)[:200]
    b = _operand(rng, 120, 200, 700, dtype, np.array([0.0, 2.0]))
    Bt = _tiled(pkg, ctx, 120, 200, b, dtype)
    for accum in (None, "plus"):
        Z = A.assign(Bt, RI, CJ, accum=accum)
        s = ar.assign(rows, cols, (I, J, V), b, RI, CJ, accum)
        oz = oracle.Csr(rows, cols, s[0], s[1], s[2].astype(np.float64))
        for X, Y, ox, oy in ((Z, A, oz, oa), (A, Z, oa, oz), (Z, Z, oz, oz)):
            p = pkg.CPlan(ctx, X, Y)
            p.spgemm()
            got, want = p.export_csr(), oracle.csr_spgemm(ox, oy, f32=f32).arrays()
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), "structure"
            assert _same_vals(got[2], np.asarray(want[2]).astype(dtype)), "values"
        pm = pkg.CPlan(ctx, A, A, mask=Z)                  # Z as a structural mask of A*A
        pm.spgemm()
        fr, fc, fv = (np.asarray(x) for x in oracle.csr_spgemm(oa, oa, f32=f32).arrays())
        fI = np.repeat(np.arange(rows, dtype=np.int32), np.diff(fr))
        inZ = np.isin(fI.astype(np.int64) * cols + fc, s[0].astype(np.int64) * cols + s[1])
        mr, mc, mv = pm.export_csr()
        assert np.array_equal(np.diff(mr), np.bincount(fI[inZ], minlength=rows)) and np.array_equal(mc, np.asarray(fc)[inZ])
        assert _same_vals(mv, np.asarray(fv)[inZ].astype(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_result_through_save_load_select_and_mxv(pkg, ctx, dtype, tmp_path):
    rows, cols, I, J, V, _ = CASES["rect_70x40_AAt"]
    c = _canonical(I, J, np.asarray(V, dtype), cols)
    Ct = _tiled(pkg, ctx, rows, cols, c, dtype)
    rng = np.random.default_rng(4)
    RI, CJ = rng.permutation(rows)[:33], rng.permutation(cols)[:18]
    a = _operand(rng, 33, 18, 120, dtype, np.array([0.0, 2.0]))
    Z = Ct.assign(_tiled(pkg, ctx, 33, 18, a, dtype), RI, CJ)
    F = _want(pkg, ctx, rows, cols, c, a, RI, CJ, None, dtype)
    assert Z.conv_ms > 0
    path = str(tmp_path / "z.pemtile")
    Z.save(path)
    _assert_same_tiling(pkg.Tiled.load(ctx, path), Z, "save / load")
    _assert_same_tiling(Z.select("triu", -2), F.select("triu", -2), "select of the result")
    _assert_same_tiling(Z.transpose(), F.transpose(), "transpose of the result")
    _assert_same_tiling(pkg.Tiled.ewise(Z, Ct, "times"), pkg.Tiled.ewise(F, Ct, "times"), "ewise of the result")
    for tr in (False, True):
        x = torch.as_tensor(rng.normal(size=Z.rows if tr else Z.cols).astype(dtype), device="cuda")
        assert _same_vals(_mxv(ctx, Z, x, tr), _mxv(ctx, F, x, tr)), f"mxv transpose={tr}"
    X = torch.as_tensor(rng.normal(size=(cols, 3)).astype(dtype), device="cuda")
    Yz, Yf = Z.spmm(X), F.spmm(X)
    ctx.synchronize()                                     # (spmm never waits; the context runs on a stream of its own)
    assert _same_vals(Yz.cpu().numpy(), Yf.cpu().numpy()), "spmm"
    for x, y in zip(Z.export_csr(), F.export_csr()):
        assert _same(x, y)
    V2 = rng.normal(size=Z.nnz).astype(dtype)
    Z.set_values(V2)
    F.set_values(V2)
    ctx.synchronize()
    _assert_same_tiling(Z, F, "set_values on the result")


# ---- 6. refresh ------------------------------------------------------------------------------------------------------------------
def _left(pkg, c, n, dtype):
    """a 24 x n operand for a plan whose B is an n-row tiling"""
    rng = np.random.default_rng(n)
    key = np.sort(rng.choice(24 * n, min(24 * n, 6 * n), replace=False))
    return pkg.Tiled.from_coo(c, 24, n, (key // n).astype(np.int32), (key % n).astype(np.int32), rng.normal(size=len(key)).astype(dtype), dtype=dtype)


def _refresh_rounds(pkg, c, ref_ctx, dtype, aged, name="powerlaw_600"):
    """set_values on C, on A or on both (row and column order), then the refresh, against a fresh assign: array for array, vals_t
    through mxv(transpose=True) and through a plan's B side"""
    rows, cols, I, J, V, _ = CASES[name]
    cI, cJ, cV = _canonical(I, J, np.asarray(V, dtype), cols)
    rng = np.random.default_rng(41)
    RI, CJ = rng.permutation(rows)[: rows // 2], rng.permutation(cols)[: cols - 7]
    ni, nj = len(RI), len(CJ)
    aI, aJ, aV = _operand(rng, ni, nj, len(I) // 2, dtype, np.array([2.0]))
    Ct, At = pkg.Tiled.from_coo(c, rows, cols, cI, cJ, cV, dtype=dtype), pkg.Tiled.from_coo(c, ni, nj, aI, aJ, aV, dtype=dtype)
    made = {"none": lambda X, Y: X.assign(Y, RI, CJ), "plus": lambda X, Y: X.assign(Y, _dev(RI), CJ, accum="plus"),
            "rows": lambda X, Y: X.assign(Y, RI, None, accum="min")}
    wide = lambda Y: Y.extract(None, np.arange(cols) % nj)   # an ni x cols operand (itself refreshed from A) for the rows-only assign
    srcA = {"none": At, "plus": At, "rows": wide(At)}
    Z = {k: f(Ct, srcA[k]) for k, f in made.items()}
    x = torch.as_tensor(rng.normal(size=rows).astype(dtype), device="cuda")
    torch.cuda.synchronize()
    if aged:                                              # handles that already hold vmap_t and the column schedule
        for t in Z.values():
            t.mxv(x, transpose=True)
            t.set_values(rng.normal(size=t.nnz))
    down = {k: pkg.CPlan(c, _left(pkg, c, rows, dtype), t) for k, t in Z.items()}   # Z as B: step 3 reads vals_t
    for p in down.values():
        p.spgemm()

    def col_to_row(I_, J_, nr, V2):                       # V2 ordered by (col, row): back to row order
        o = np.argsort(J_.astype(np.int64) * nr + I_, kind="stable")
        out = np.empty_like(V2)
        out[o] = V2
        return out

    for rnd, (new_c, new_a, order) in enumerate(((True, False, "row"), (False, True, "col"), (True, True, "col"), (True, True, "row"))):
        if new_c:
            V2 = rng.normal(size=Ct.nnz)
            Ct.set_values(V2, order)
            cV = (V2 if order == "row" else col_to_row(cI, cJ, rows, V2)).astype(dtype)
        if new_a:
            V2 = rng.normal(size=At.nnz)
            At.set_values(V2, order)
            aV = (V2 if order == "row" else col_to_row(aI, aJ, ni, V2)).astype(dtype)
            srcA["rows"].set_values_from_extract(At)
        Fc, Fa = pkg.Tiled.from_coo(ref_ctx, rows, cols, cI, cJ, cV, dtype=dtype), pkg.Tiled.from_coo(ref_ctx, ni, nj, aI, aJ, aV, dtype=dtype)
        for k, t in Z.items():
            t.set_values_from_assign(Ct, srcA[k])
            c.synchronize()
            F = made[k](Fc, wide(Fa) if k == "rows" else Fa)
            _assert_same_accum(t, F, f"refresh {k} round {rnd}", "min" if k == "rows" else "plus")
            assert _same_vals(_mxv(c, t, x, True), _mxv(ref_ctx, F, x, True)), f"{k}: vals_t by mxv"
            down[k].step3()
            fresh = pkg.CPlan(ref_ctx, _left(pkg, ref_ctx, rows, dtype), F)
            fresh.spgemm()
            for g, w in zip(down[k].export_csr(), fresh.export_csr()):
                assert _same(g, w), f"{k}: the B side of a plan"


@pytest.mark.parametrize("aged", (False, True), ids=("fresh", "aged"))
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_refresh_equals_fresh(pkg, ctx, dtype, aged):
    _refresh_rounds(pkg, ctx, ctx, dtype, aged)


def test_refresh_on_a_graph_replay_context(pkg, ctx):
    g = pkg.Context(0)
    try:
        g.set_graph_replay(True)
        rows, cols, I, J, V, _ = CASES["band_1500"]
        cI, cJ, cV = _canonical(I, J, np.asarray(V), cols)
        rng = np.random.default_rng(8)
        p = rng.permutation(rows)[:700]
        a = _operand(rng, 700, 700, 3000, np.float64, np.array([2.0]))
        Ct, At = pkg.Tiled.from_coo(g, rows, cols, cI, cJ, cV), _tiled(pkg, g, 700, 700, a, np.float64)
        Z = Ct.assign(At, p, p, accum="plus")
        pz = pkg.CPlan(g, Z, Ct)
        for _ in range(3):
            pz.spgemm()                                   # captured, then replayed
        for seed in (21, 22, 23):
            r2 = np.random.default_rng(seed)
            V2, W2 = r2.normal(size=Ct.nnz), r2.normal(size=At.nnz)
            Ct.set_values(V2)
            At.set_values(W2)
            Z.set_values_from_assign(Ct, At)
            pz.spgemm()
            C2, A2 = pkg.Tiled.from_coo(ctx, rows, cols, cI, cJ, V2), pkg.Tiled.from_coo(ctx, 700, 700, a[0], a[1], W2)
            fz = pkg.CPlan(ctx, C2.assign(A2, p, p, accum="plus"), C2)
            fz.spgemm()
            for x, y in zip(pz.export_csr(), fz.export_csr()):
                assert _same(x, y), seed
    finally:
        g.close()


def test_refresh_on_a_stream_context(pkg, ctx):
    prev = torch.cuda.current_stream()
    stream = torch.cuda.Stream()                          # (not the null stream: the context would make its own)
    g = pkg.Context(0, stream=stream.cuda_stream)
    try:
        torch.cuda.set_stream(stream)
        _refresh_rounds(pkg, g, ctx, np.float64, aged=True, name="rand_300")
    finally:
        torch.cuda.set_stream(prev)
        g.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_handle_unchanged(pkg, ctx):
    L = pkg.lib()
    rows, cols, I, J, V, _ = CASES["rect_70x40_AAt"]
    Ct = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    rng = np.random.default_rng(2)
    A32 = _tiled(pkg, ctx, 3, 2, _operand(rng, 3, 2, 4, np.float64), np.float64)
    A32f = _tiled(pkg, ctx, 3, 2, _operand(rng, 3, 2, 4, np.float32), np.float32)
    Afull = _tiled(pkg, ctx, rows, cols, _operand(rng, rows, cols, 50, np.float64), np.float64)
    snaps = {k: _snapshot(t) for k, t in (("C", Ct), ("A", A32))}
    h = C.c_void_p()
    ctx.synchronize()
    before = ctx.memory_stats()["in_use_bytes"]

    def host(I_, ni, J_, nj, accum=-1, out=True, c=Ct._h, a=A32._h, cx=ctx._h):
        pi = None if I_ is None else np.ascontiguousarray(I_, np.int32)
        pj = None if J_ is None else np.ascontiguousarray(J_, np.int32)
        return L.pem_tiled_assign(cx, c, a, None if pi is None else pi.ctypes.data_as(C.c_void_p), C.c_int64(ni),
                                  None if pj is None else pj.ctypes.data_as(C.c_void_p), C.c_int64(nj), accum, C.byref(h) if out else None)

    def device(I_, ni, J_, nj, accum=-1, out=True, c=Ct._h, a=A32._h, cx=ctx._h):
        di, dj = _dev(I_), _dev(J_)
        torch.cuda.synchronize()
        return L.pem_tiled_assign_device(cx, c, a, None if di is None else C.c_void_p(di.data_ptr()), C.c_int64(ni),
                                         None if dj is None else C.c_void_p(dj.data_ptr()), C.c_int64(nj), accum, C.byref(h) if out else None)

    for fn in (host, device):
        for bad_i, bad_j in (([0, -1, 3], [0, 1]), ([0, rows, 3], [0, 1]), ([0, 1, 2], [cols, 0]), ([0, 1, 2], [1, -1]),
                             ([2 ** 31 - 1, 0, 1], [0, 1]), ([-(2 ** 31), 0, 1], [0, 1]),
                             ([4, 9, 4], [0, 1]), ([0, 1, 2], [7, 7])):                     # out of range; repeated
            h.value = 12345
            assert fn(bad_i, 3, bad_j, 2) == PEM_E_INVALID and h.value is None, (fn.__name__, bad_i, bad_j)
        for ni, nj in ((0, 2), (3, 0), (-3, 2), (2 ** 31, 2)):       # n < 1 or n > INT32_MAX with a non-null list
            h.value = 12345
            assert fn([0, 1, 2], ni, [0, 1], nj) == PEM_E_INVALID and h.value is None, (fn.__name__, ni, nj)
        for accum in (-2, 6, 100):
            h.value = 12345
            assert fn([0, 1, 2], 3, [0, 1], 2, accum=accum) == PEM_E_INVALID and h.value is None, (fn.__name__, accum)
        for bi, bj in (([0, 1], [0, 1]), ([0, 1, 2], [0, 1, 2]), (None, [0, 1]), ([0, 1, 2], None), (None, None)):   # A is 3 x 2
            h.value = 12345
            assert fn(bi, 0 if bi is None else len(bi), bj, 0 if bj is None else len(bj)) == PEM_E_INVALID and h.value is None, (fn.__name__, bi, bj)
        h.value = 12345
        assert fn([0, 1, 2], 3, [0, 1], 2, a=A32f._h) == PEM_E_INVALID and h.value is None      # different value types
        assert fn([0, 1, 2], 3, [0, 1], 2, out=False) == PEM_E_INVALID
        assert fn([0, 1, 2], 3, [0, 1], 2, c=None) == PEM_E_INVALID
        assert fn([0, 1, 2], 3, [0, 1], 2, a=None) == PEM_E_INVALID
        assert fn([0, 1, 2], 3, [0, 1], 2, cx=None) == PEM_E_INVALID
        for k, t in (("C", Ct), ("A", A32)):
            _unchanged(pkg, t, snaps[k], fn.__name__ + " " + k)
        ctx.synchronize()
        assert ctx.memory_stats()["in_use_bytes"] == before, fn.__name__
    f = L.pem_tiled_set_values_from_assign
    assert f(None, Ct._h, Ct._h, Ct._h) == PEM_E_INVALID and f(ctx._h, None, Ct._h, Ct._h) == PEM_E_INVALID
    assert f(ctx._h, Ct._h, None, Ct._h) == PEM_E_INVALID and f(ctx._h, Ct._h, Ct._h, None) == PEM_E_INVALID
    assert host(None, 77, None, -5, a=Afull._h) == 0      # null lists are "all": their counts are ignored
    _assert_same_tiling(pkg.Tiled(ctx, C.c_void_p(h.value)), Afull, "C(:, :) = A")
    # the Python layer
    for bad in ([-1, 0, 1], [rows, 0, 1], [0.5, 1, 2], [[0, 1, 2]], [1, 1, 2]):
        with pytest.raises(ValueError):
            Ct.assign(A32, bad, [0, 1])
    with pytest.raises(ValueError):
        Ct.assign(A32, [0, 1, 2], [5, 5])
    with pytest.raises(ValueError):
        Ct.assign(A32, [0, 1, 2], [0, 1], accum="second")
    with pytest.raises(ValueError):
        Ct.assign(A32, [0, 1, 2], torch.zeros(2, dtype=torch.int64, device="cuda"))
    with pytest.raises(pkg.PemError) as e:
        Ct.assign(A32, torch.tensor([3, 8, 3], dtype=torch.int32, device="cuda"), [0, 1])     # a repeat in a device list
    assert e.value.status == PEM_E_INVALID and "repeat" in str(e.value)
    with pytest.raises(pkg.PemError) as e:
        Ct.assign(A32, [0, 1, 2], torch.tensor([0, cols], dtype=torch.int32, device="cuda"))
    assert e.value.status == PEM_E_INVALID
    with pytest.raises(pkg.PemError) as e:
        Ct.assign(A32, [0, 1], [0, 1])
    assert e.value.status == PEM_E_INVALID
    for k, t in (("C", Ct), ("A", A32)):
        _unchanged(pkg, t, snaps[k], "python refusals " + k)


def test_refresh_refusals(pkg, ctx):
    rows, cols, I, J, V, _ = CASES["rand_300"]
    Ct = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    A = Ct.extract(np.arange(100), np.arange(100))
    p = np.arange(100, 200)
    Z, E, R = Ct.assign(A, p, p), pkg.Tiled.ewise(Ct, Ct, "plus"), Ct.extract(p, p)
    snaps = {k: _snapshot(t) for k, t in (("Z", Z), ("E", E), ("R", R), ("C", Ct), ("A", A))}
    C2 = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)     # same matrix, another tiling
    S = pkg.Tiled.ewise(A, A, "plus").select("tril", 1000)   # a 100 x 100 tiling not made from C
    for call in (lambda: Z.set_values_from_assign(A, Ct),                                    # swapped
                 lambda: Z.set_values_from_assign(C2, A), lambda: Z.set_values_from_assign(Ct, S),   # another tiling
                 lambda: Z.set_values_from_ewise(Ct, A), lambda: Z.set_values_from_extract(Ct), lambda: Z.set_values_from_select(Ct),
                 lambda: E.set_values_from_assign(Ct, Ct), lambda: R.set_values_from_assign(Ct, A), lambda: Ct.set_values_from_assign(Ct, A)):
        with pytest.raises(pkg.PemError) as e:
            call()
        assert e.value.status == PEM_E_INVALID
    for k, t in (("Z", Z), ("E", E), ("R", R), ("C", Ct), ("A", A)):
        _unchanged(pkg, t, snaps[k], k)
    Z.set_values_from_assign(Ct, A)                       # the right sources
    ctx.synchronize()
    _unchanged(pkg, Z, snaps["Z"], "a refresh from unchanged values")
    A.close()                                             # a tiling recreated (possibly at the same address)
    A3 = Ct.extract(np.arange(100), np.arange(100))
    with pytest.raises(pkg.PemError):
        Z.set_values_from_assign(Ct, A3)


# ---- 8. empty operands and results; determinism ----------------------------------------------------------------------------------
def test_empty_operands_and_results(pkg, ctx):
    E = _empty(pkg, ctx, 40, 30, np.float64)
    for Z in (E.assign(E), E.assign(_empty(pkg, ctx, 3, 2, np.float64), [5, 39, 0], [29, 1]), E.assign(_empty(pkg, ctx, 1, 30, np.float64), [7], None),
              E.assign(E, accum="plus"), E.assign(_empty(pkg, ctx, 40, 1, np.float64), None, [0], accum="land")):
        assert (Z.rows, Z.cols) == (40, 30) and Z.nnz == 0 and Z.ntiles == 0
        rp, ci, v = Z.export_csr()
        assert np.array_equal(rp, np.zeros(41, np.int32)) and len(ci) == len(v) == 0
    Z = E.assign(E)
    Z.set_values_from_assign(E, E)                        # the refresh of an empty result is a no-op
    rows, cols, I, J, V, _ = CASES["rand_50"]
    Ct = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    X = Ct.assign(_empty(pkg, ctx, rows, cols, np.float64))   # the whole of C deleted
    assert X.nnz == 0 and X.ntiles == 0
    p = pkg.CPlan(ctx, X, Ct)
    p.spgemm()
    assert p.info()["nnz_c"] == 0
    one = _tiled(pkg, ctx, 1, 1, (np.zeros(1, np.int32), np.zeros(1, np.int32), np.array([0.0])), np.float64)
    Y = X.assign(one, [49], [49])                         # an explicit zero stays an entry
    assert Y.nnz == 1 and Y.ntiles == 1
    Y = Ct.assign(pkg.Tiled.ewise(Ct, Ct, "plus", alpha=-2.0), accum="plus")   # results that come out as 0 stay entries
    assert Y.nnz == Ct.nnz and not np.any(Y.array("vals"))


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_two_calls_give_identical_bytes(pkg, ctx, dtype):
    rows, cols, I, J, V, _ = CASES["hub_row_4000"]
    Ct = pkg.Tiled.from_coo(ctx, rows, cols, I, J, _with_specials(CASES["hub_row_4000"]).astype(dtype), dtype=dtype)
    rng = np.random.default_rng(6)
    RI, CJ = rng.permutation(rows)[:2500], rng.permutation(cols)[:3000]
    At = _tiled(pkg, ctx, 2500, 3000, _operand(rng, 2500, 3000, 9000, dtype), dtype)
    for make in (lambda: Ct.assign(At, RI, CJ), lambda: Ct.assign(At, _dev(RI), _dev(CJ), accum="plus"), lambda: Ct.assign(At, RI, _dev(CJ), accum="min")):
        X, Y = make(), make()
        for n in ARRAYS:
            assert X.array(n).tobytes() == Y.array(n).tobytes(), n
        X.set_values_from_assign(Ct, At)
        ctx.synchronize()
        for n in ARRAYS:
            assert X.array(n).tobytes() == Y.array(n).tobytes(), n + " after a refresh"
