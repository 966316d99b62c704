"""GPU: element-wise combination of tilings (pem_tiled_ewise), its refresh (pem_tiled_set_values_from_ewise) and the tiling export
(pem_tiled_export_csr).

The central check: the tiling made on the device equals, array for array, the tiling pem_tiled_from_coo builds from ewiseref's COO
of the same operands -- values bit for bit, except that NaN is compared as NaN and zero signs are ignored under min / max.
"""
import os

import numpy as np
import pytest
import torch

import ewiseref as er
import semiringref as sr
from matgen import cases, random_coo

pytestmark = pytest.mark.gpu

torch.cuda.is_available()   # (torch's runtime first, as in the other GPU files)

CASES = cases()
PEM_E_INVALID = -1
DTYPES = (np.float64, np.float32)
INFO = ("rows", "cols", "nnz", "tile_rows", "tile_cols", "ntiles", "value_bytes")
ARRAYS = ("tile_keys", "tile_nnz_ptr", "masks", "rowptr", "rowcolidx", "vals", "masks_t", "tile_rowptr", "tile_colidx", "tile_colptr",
          "tile_rowidx", "tile_offsets")
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 2.0])


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32) if a.dtype.kind == "f" else a


def _same_vals(got, want, op):
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


def _second(case, seed=7):
    """a second seeded operand of the case's shape: about half of A's positions, and as many others; some special values"""
    rows, cols, I, J, V, _ = case
    rng = np.random.default_rng(seed + rows * 131 + cols)
    ka = I.astype(np.int64) * cols + J
    keep = ka[rng.random(len(ka)) < 0.5]
    other = rng.choice(rows * cols, size=min(len(ka) + 1, rows * cols), replace=False)
    k = np.unique(np.concatenate([keep, other]))
    W = rng.uniform(-2.0, 2.0, len(k))
    sp = rng.random(len(k)) < 0.1
    W[sp] = rng.choice(SPECIAL, int(sp.sum()))
    return (k // cols).astype(np.int32), (k % cols).astype(np.int32), W


def _operands(pkg, ctx, case, kind, dtype):
    """A and B tilings plus their canonical COO triples (in dtype).  kind: 'self' (B is A), 'second', 'transposed' (B a transpose=1
    tiling of the second operand's transpose)"""
    rows, cols, I, J, V, _ = case
    a = er.canonical(I, J, np.asarray(V, dtype), cols)
    A = pkg.Tiled.from_coo(ctx, rows, cols, *a, dtype=dtype)
    if kind == "self":
        return A, A, a, a
    b = er.canonical(*_second(case), cols)
    b = (b[0], b[1], b[2].astype(dtype))
    if kind == "second":
        B = pkg.Tiled.from_coo(ctx, rows, cols, *b, dtype=dtype)
    else:
        B = pkg.Tiled.from_coo(ctx, cols, rows, b[1], b[0], b[2], True, dtype=dtype)
    return A, B, a, b


def _expect(pkg, ctx, rows, cols, a, b, op, pattern, alpha, beta, dtype):
    I, J, V = er.ewise(cols, a, b, op, pattern, alpha, beta)
    return pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=dtype), (I, J, V)


def _check(pkg, ctx, case, kind, dtype, op, pattern, alpha=1.0, beta=1.0, label=""):
    rows, cols = case[0], case[1]
    A, B, a, b = _operands(pkg, ctx, case, kind, dtype)
    R = pkg.Tiled.ewise(A, B, op=op, pattern=pattern, alpha=alpha, beta=beta)
    want, _ = _expect(pkg, ctx, rows, cols, a, b, op, pattern, alpha, beta, dtype)
    _assert_same_tiling(R, want, f"{label} {kind} {op} {pattern} {alpha},{beta}", op)
    return R


# ---- equality with ewiseref + from_coo ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("kind", ("self", "second", "transposed"))
@pytest.mark.parametrize("name", sorted(CASES))
def test_plain_pairs_every_case(pkg, ctx, name, kind, dtype):
    for pattern in er.PATTERNS:
        _check(pkg, ctx, CASES[name], kind, dtype, "plus", pattern, label=name)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", ("rand_300", "powerlaw_600", "ragged_37", "dense_48", "cancel_and_zero", "rect_70x40_AAt"))
def test_ops_patterns_scales(pkg, ctx, name, dtype):
    for op in er.OPS:
        for pattern in er.PATTERNS:
            for alpha, beta in ((1.0, 1.0), (2.5, -0.75), (0.1, 0.0)):
                _check(pkg, ctx, CASES[name], "second", dtype, op, pattern, alpha, beta, label=name)


# ---- edge cases ----------------------------------------------------------------------------------------------------------------
def test_disjoint_patterns(pkg, ctx):
    rows = cols = 40
    a = er.canonical(np.arange(20, dtype=np.int32), np.arange(20, dtype=np.int32), np.arange(1.0, 21.0), cols)
    b = er.canonical(np.arange(20, 40, dtype=np.int32), np.arange(20, dtype=np.int32), np.arange(-20.0, 0.0), cols)
    A, B = pkg.Tiled.from_coo(ctx, rows, cols, *a), pkg.Tiled.from_coo(ctx, rows, cols, *b)
    U = pkg.Tiled.ewise(A, B)
    _assert_same_tiling(U, _expect(pkg, ctx, rows, cols, a, b, "plus", "union", 1.0, 1.0, np.float64)[0], "disjoint union")
    X = pkg.Tiled.ewise(A, B, pattern="intersect")
    assert X.nnz == 0 and X.ntiles == 0 and X.rows == rows and X.cols == cols
    rp, ci, v = X.export_csr()
    assert np.array_equal(rp, np.zeros(rows + 1, np.int32)) and len(ci) == len(v) == 0
    # the empty result works as an operand: of a plan, of another ewise
    p = pkg.CPlan(ctx, X, A)
    p.spgemm()
    assert p.info()["nnz_c"] == 0
    Y = pkg.Tiled.ewise(X, A)
    _assert_same_tiling(Y, A, "empty (+) A")
    Z = pkg.Tiled.ewise(A, X)                              # ... and as B (the union with no B tiles)
    _assert_same_tiling(Z, A, "A (+) empty")
    W = pkg.Tiled.ewise(A, X, op="times", pattern="intersect")
    assert W.nnz == 0 and W.ntiles == 0
    Z.set_values_from_ewise(A, X)                          # the refresh of a union with an empty side
    ctx.synchronize()
    _assert_same_tiling(Z, A, "A (+) empty, refreshed")


def test_full_tiles_both_sides(pkg, ctx):
    rows = cols = 48
    I, J = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    I, J = I.ravel().astype(np.int32), J.ravel().astype(np.int32)
    rng = np.random.default_rng(3)
    a = er.canonical(I, J, rng.normal(size=len(I)), cols)
    b = er.canonical(I, J, rng.normal(size=len(I)), cols)
    A, B = pkg.Tiled.from_coo(ctx, rows, cols, *a), pkg.Tiled.from_coo(ctx, rows, cols, *b)
    for op in er.OPS:
        for pattern in er.PATTERNS:
            R = pkg.Tiled.ewise(A, B, op=op, pattern=pattern)
            _assert_same_tiling(R, _expect(pkg, ctx, rows, cols, a, b, op, pattern, 1.0, 1.0, np.float64)[0], f"full {op} {pattern}", op)


def test_ragged_shape(pkg, ctx):
    case = random_coo(np.random.default_rng(11), 45, 29, 300) + (False,)
    for op in ("plus", "max"):
        _check(pkg, ctx, case, "second", np.float64, op, "union", label="45x29")
        _check(pkg, ctx, case, "transposed", np.float32, op, "intersect", label="45x29")


def test_one_tile_row_holding_every_tile(pkg, ctx):
    """16 x 65536 with an entry in every tile column: the tile matching searches one long tile row"""
    rows, cols = 16, 65536
    rng = np.random.default_rng(5)
    tc = np.arange(cols // 16)
    Ia = rng.integers(0, 16, len(tc)).astype(np.int32)
    Ja = (tc * 16 + rng.integers(0, 16, len(tc))).astype(np.int32)
    keep = rng.random(len(tc)) < 0.5                   # B: the same positions on half the tile columns, other ones elsewhere
    Ib = np.where(keep, Ia, (Ia + 3) % 16).astype(np.int32)
    Jb = np.where(keep, Ja, tc * 16 + (Ja + 5) % 16).astype(np.int32)
    b_cols = rng.random(len(tc)) < 0.8                 # ... and B leaves out some tile columns
    a = er.canonical(Ia, Ja, rng.normal(size=len(Ia)), cols)
    b = er.canonical(Ib[b_cols], Jb[b_cols], rng.normal(size=int(b_cols.sum())), cols)
    A, B = pkg.Tiled.from_coo(ctx, rows, cols, *a), pkg.Tiled.from_coo(ctx, rows, cols, *b)
    for pattern in er.PATTERNS:
        R = pkg.Tiled.ewise(A, B, op="times", pattern=pattern, alpha=0.5)
        _assert_same_tiling(R, _expect(pkg, ctx, rows, cols, a, b, "times", pattern, 0.5, 1.0, np.float64)[0], f"one tile row {pattern}")


# ---- errors ---------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments(pkg, ctx):
    import ctypes as C
    L = pkg.lib()
    case = CASES["rand_50"]
    A, B, _, _ = _operands(pkg, ctx, case, "second", np.float64)
    A32 = pkg.Tiled.from_coo(ctx, case[0], case[1], case[2], case[3], case[4], dtype=np.float32)
    other = pkg.Tiled.from_coo(ctx, 50, 49, np.array([1], np.int32), np.array([2], np.int32), np.array([1.0]))
    h = C.c_void_p()

    def call(a, b, pattern=0, op=0, out=True):
        return L.pem_tiled_ewise(ctx._h, a, b, pattern, op, C.c_double(1.0), C.c_double(1.0), C.byref(h) if out else None)

    assert call(A._h, other._h) == PEM_E_INVALID            # shape
    assert call(A._h, A32._h) == PEM_E_INVALID              # value type
    assert call(A._h, B._h, op=6) == PEM_E_INVALID
    assert call(A._h, B._h, op=-1) == PEM_E_INVALID
    assert call(A._h, B._h, pattern=2) == PEM_E_INVALID
    assert call(None, B._h) == PEM_E_INVALID
    assert call(A._h, None) == PEM_E_INVALID
    assert call(A._h, B._h, out=False) == PEM_E_INVALID
    assert L.pem_tiled_ewise(None, A._h, B._h, 0, 0, C.c_double(1.0), C.c_double(1.0), C.byref(h)) == PEM_E_INVALID
    with pytest.raises(ValueError):
        pkg.Tiled.ewise(A, B, op="minus")
    with pytest.raises(ValueError):
        pkg.Tiled.ewise(A, B, pattern="xor")
    # the tiling export refuses the other value type
    n = C.c_int64()
    rp = np.zeros(A.rows + 1, np.int32)
    assert L.pem_tiled_export_csr_f32(ctx._h, A._h, C.byref(n), rp.ctypes.data_as(C.c_void_p), None, None) == PEM_E_INVALID
    assert L.pem_tiled_export_csr(ctx._h, A32._h, C.byref(n), rp.ctypes.data_as(C.c_void_p), None, None) == PEM_E_INVALID


# ---- alpha*A*B + beta*D ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", ("rand_300", "powerlaw_600", "ragged_37", "cancel_and_zero"))
def test_axpby_against_oracle(pkg, oracle, ctx, name, dtype):
    rows, cols, I, J, V, _ = CASES[name]
    f32 = dtype == np.float32
    Vq = V.astype(np.float32).astype(np.float64) if f32 else V
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=dtype)
    plan = pkg.CPlan(ctx, A, A)
    plan.spgemm()
    Ct = pkg.Tiled.from_cplan(plan)
    d = er.canonical(*_second(CASES[name], 19), cols)
    d = (d[0], d[1], d[2].astype(dtype))
    D = pkg.Tiled.from_coo(ctx, rows, cols, *d, dtype=dtype)
    R = pkg.Tiled.ewise(Ct, D, op="plus", alpha=2.0, beta=-0.5)
    oa = oracle.Csr(rows, cols, I, J, Vq)
    rp, ci, v = oracle.csr_spgemm(oa, oa, f32=f32).arrays()
    c = (np.repeat(np.arange(rows, dtype=np.int32), np.diff(rp)), ci.astype(np.int32), np.asarray(v).astype(dtype))
    want, coo = _expect(pkg, ctx, rows, cols, c, d, "plus", "union", 2.0, -0.5, dtype)
    _assert_same_tiling(R, want, f"{name} 2 A A - 0.5 D")
    grp, gci, gv = R.export_csr()
    assert np.array_equal(np.diff(grp), np.bincount(coo[0], minlength=rows)) and np.array_equal(gci, coo[1])
    assert _same_vals(gv, coo[2], "plus")


@pytest.mark.parametrize("name", ("rand_300", "powerlaw_600", "band_1500"))
def test_min_plus_relaxation(pkg, ctx, name):
    """D <- min(D, D (x) D) under min-plus, one step, against semiringref"""
    rows, cols, I, J, V, _ = CASES[name]
    W = np.abs(np.asarray(V)) + 0.5
    D = pkg.Tiled.from_coo(ctx, rows, cols, I, J, W)
    plan = pkg.CPlan(ctx, D, D, semiring="min_plus")
    plan.spgemm()
    C2 = pkg.Tiled.from_cplan(plan)
    R = pkg.Tiled.ewise(D, C2, op="min")
    a = sr.coo_to_csr(rows, cols, I, J, W)
    c = sr.spgemm(a, a, cols, "min_plus", np.float64)
    ci_rows = np.repeat(np.arange(rows), np.diff(c[0]))
    d = er.canonical(I, J, W, cols)
    cc = er.canonical(ci_rows, c[1], c[2], cols)
    Iw, Jw, Vw = er.ewise(cols, d, cc, "min", "union")
    rp, ci, v = R.export_csr()
    assert np.array_equal(ci, Jw) and np.array_equal(np.diff(rp), np.bincount(Iw, minlength=rows))
    assert sr.same_values(v, Vw)


# ---- refresh -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("op,pattern", (("plus", "union"), ("times", "intersect"), ("min", "union"), ("land", "union")))
def test_refresh_equals_fresh(pkg, ctx, op, pattern, dtype):
    case = CASES["powerlaw_600"]
    A, B, a, b = _operands(pkg, ctx, case, "second", dtype)
    R = pkg.Tiled.ewise(A, B, op=op, pattern=pattern, alpha=1.5, beta=-2.0)
    rng = np.random.default_rng(23)
    for which in ("A", "B", "AB"):
        if "A" in which:
            A.set_values(rng.normal(size=A.nnz))
        if "B" in which:
            B.set_values(rng.normal(size=B.nnz))
        R.set_values_from_ewise(A, B)
        ctx.synchronize()
        F = pkg.Tiled.ewise(A, B, op=op, pattern=pattern, alpha=1.5, beta=-2.0)
        _assert_same_tiling(R, F, f"refresh {which}", op)
        # vals_t: R as the B of a plan gives what the fresh tiling gives
        p1, p2 = pkg.CPlan(ctx, A, R), pkg.CPlan(ctx, A, F)
        p1.spgemm()
        p2.spgemm()
        for x, y in zip(p1.export_csr(), p2.export_csr()):
            assert _same_vals(x, y, op) if x.dtype.kind == "f" else np.array_equal(x, y)


def test_refresh_through_chain(pkg, oracle, ctx):
    """new A -> step 3 -> set_values_from_cplan -> set_values_from_ewise, against the oracle"""
    rows, cols, I, J, V, _ = CASES["rand_300"]
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    plan = pkg.CPlan(ctx, A, A)
    plan.spgemm()
    Ct = pkg.Tiled.from_cplan(plan)
    d = er.canonical(*_second(CASES["rand_300"], 29), cols)
    D = pkg.Tiled.from_coo(ctx, rows, cols, *d)
    R = pkg.Tiled.ewise(Ct, D, alpha=3.0)
    V2 = np.random.default_rng(31).normal(size=len(V))
    a_sorted = er.canonical(I, J, V2, cols)
    A.set_values(a_sorted[2])
    plan.step3()
    Ct.set_values_from_cplan(plan)
    R.set_values_from_ewise(Ct, D)
    ctx.synchronize()
    oa = oracle.Csr(rows, cols, *a_sorted)
    rp, ci, v = oracle.csr_spgemm(oa, oa).arrays()
    c = (np.repeat(np.arange(rows, dtype=np.int32), np.diff(rp)), ci.astype(np.int32), np.asarray(v))
    _assert_same_tiling(R, _expect(pkg, ctx, rows, cols, c, d, "plus", "union", 3.0, 1.0, np.float64)[0], "chain refresh")
    # used as B of a plan (reads vals_t), against the oracle
    p = pkg.CPlan(ctx, A, R)
    p.spgemm()
    rrp, rci, rv = R.export_csr()
    orr = oracle.Csr(rows, cols, np.repeat(np.arange(rows, dtype=np.int32), np.diff(rrp)), rci, rv)
    want = oracle.csr_spgemm(oa, orr).arrays()
    got = p.export_csr()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and _same_vals(got[2], np.asarray(want[2]), "plus")


def test_refresh_refuses_other_operands(pkg, ctx):
    case = CASES["rand_50"]
    A, B, a, b = _operands(pkg, ctx, case, "second", np.float64)
    R = pkg.Tiled.ewise(A, B)
    with pytest.raises(pkg.PemError) as e:
        R.set_values_from_ewise(B, A)                      # swapped
    assert e.value.status == PEM_E_INVALID
    A2 = pkg.Tiled.from_coo(ctx, case[0], case[1], *a)      # same matrix, another tiling
    with pytest.raises(pkg.PemError):
        R.set_values_from_ewise(A2, B)
    with pytest.raises(pkg.PemError):
        A.set_values_from_ewise(A, B)                      # not made by ewise
    R.set_values_from_ewise(A, B)                          # the right pair
    ctx.synchronize()
    B.close()                                              # a tiling recreated (possibly at the same address)
    B3 = pkg.Tiled.from_coo(ctx, case[0], case[1], *b)
    with pytest.raises(pkg.PemError):
        R.set_values_from_ewise(A, B3)


# ---- the result as an operand, save / load ---------------------------------------------------------------------------------------
def test_result_as_operand_mask_and_cache(pkg, oracle, ctx, tmp_path):
    case = CASES["powerlaw_600"]
    rows, cols = case[0], case[1]
    A, B, a, b = _operands(pkg, ctx, case, "second", np.float64)
    R = pkg.Tiled.ewise(A, B)
    rp, ci, v = R.export_csr()
    rI = np.repeat(np.arange(rows, dtype=np.int32), np.diff(rp))
    orr, oa = oracle.Csr(rows, cols, rI, ci, v), oracle.Csr(rows, cols, *a)
    for X, Y, ox, oy in ((R, A, orr, oa), (A, R, oa, orr), (R, R, orr, orr)):
        p = pkg.CPlan(ctx, X, Y)
        p.spgemm()
        got, want = p.export_csr(), oracle.csr_spgemm(ox, oy).arrays()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and _same_vals(got[2], np.asarray(want[2]), "plus")
    pm = pkg.CPlan(ctx, A, A, mask=R)
    pm.spgemm()
    full = pkg.CPlan(ctx, A, A)
    full.spgemm()
    fr, fc, fv = full.export_csr()
    fI = np.repeat(np.arange(rows), np.diff(fr))
    inR = np.isin(fI.astype(np.int64) * cols + fc, rI.astype(np.int64) * cols + ci)
    mr, mc, mv = pm.export_csr()
    assert np.array_equal(mc, fc[inR]) and _same_vals(mv, fv[inR], "plus")
    path = os.path.join(tmp_path, "r.pemtile")
    R.save(path)
    L = pkg.Tiled.load(ctx, path)
    _assert_same_tiling(L, R, "save / load")


# ---- tiling export -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", sorted(CASES))
def test_export_csr_every_case(pkg, ctx, name, dtype):
    import scipy.sparse as sp
    rows, cols, I, J, V, _ = CASES[name]
    Vd = np.asarray(V, dtype)
    for tr in (False, True):
        T = pkg.Tiled.from_coo(ctx, rows, cols, I, J, Vd, tr, dtype=dtype)
        m = sp.coo_matrix((Vd, (I, J)), shape=(rows, cols)).tocsr()
        if tr:
            m = m.T.tocsr()
        m.sort_indices()
        rp, ci, v = T.export_csr()
        assert v.dtype == np.dtype(dtype)
        assert np.array_equal(rp, m.indptr) and np.array_equal(ci, m.indices), f"{name} transpose={tr}: structure"
        assert np.array_equal(_bits(v), _bits(m.data.astype(dtype))), f"{name} transpose={tr}: values"
