"""GPU: the sampled sparse product of a tiling (pem_tiled_sampled_mxm / pem_tiled_set_values_sampled_mxm, INTEGRATION.md
section 3w).

Every comparison is bit for bit over every entry (NaN == NaN; +0 == -0 under min / max only): there is no tolerance and no entry
is left out.  The references: sampledref (the oracle's fma chain per entry, numpy folds for the other semirings), the masked plan
C<S> = A * B on the GPU, and a from_csr rebuild with the reference values.  Every case runs in fp64 and fp32, under the six
semirings and for both transpose_b values: with transpose_b = 1 the device gets the tiling of B^T and the product stays A * B.

S is A's pattern wherever A's shape is the product's; a non-square `_AAt` case of matgen has an m x m product, so its S is a random
m x m pattern (sampledref.problem).  long_lists: the issue lists five match positions for the longer list and four for the
shorter, but a match has one position in each; the generator uses 0, 63, 64, 65, 129 and 0, 63, 64, 65, 69.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import sampledref as sr
from matgen import hypersparse
from test_gpu_sddmm import SPECIAL

pytestmark = pytest.mark.gpu

torch.cuda.is_available()   # (torch's runtime first, as in the other GPU files)

PEM_E_INVALID, PEM_E_STATE = -1, -6
DTYPES = (np.float64, np.float32)
MINMAX = ("min_plus", "max_plus", "max_times")
NAMES = sr.SMALL + sorted(sr.GENS)
INFO = ("rows", "cols", "nnz", "tile_rows", "tile_cols", "ntiles", "value_bytes")
ARRAYS = ("tile_keys", "tile_nnz_ptr", "masks", "rowptr", "rowcolidx", "vals", "masks_t", "tile_rowptr", "tile_colidx", "tile_colptr",
          "tile_rowidx", "tile_offsets")


@pytest.fixture(scope="module")
def tctx(pkg):
    """a context on a torch stream made current for the module (as in test_gpu_spmm.py)"""
    prev = torch.cuda.current_stream()
    s = torch.cuda.Stream()
    torch.cuda.set_stream(s)
    c = pkg.Context(0, stream=s.cuda_stream)
    yield c
    c.close()
    torch.cuda.set_stream(prev)


def _same(got, want, kind="plus_times"):
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    ok = (got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want))
    if kind in MINMAX:
        ok |= (got == 0) & (want == 0)
    return bool(np.all(ok))


def _vals(T):
    return T.export_csr()[2]


def _tiling(pkg, ctx, rows, cols, M, dtype, transposed=False):
    """the tiling of the rows x cols CSR triple M -- or of its transpose"""
    I, J = sr.rows_of(M[0]).astype(np.int32), np.asarray(M[1], np.int32)
    if transposed:
        return pkg.Tiled.from_coo(ctx, cols, rows, J, I, M[2], dtype=dtype)
    return pkg.Tiled.from_coo(ctx, rows, cols, I, J, M[2], dtype=dtype)


def _pattern_tiling(pkg, ctx, m, p, S, dtype):
    return pkg.Tiled.from_coo(ctx, m, p, S[0].astype(np.int32), S[1].astype(np.int32), np.ones(len(S[0])), dtype=dtype)


_PROBLEMS = {}


def _problem(name):
    """sampledref.problem(name) and its matched pairs, computed once for the module and left unchanged"""
    if name not in _PROBLEMS:
        m, n, p, S, A, B = sr.problem(name)
        _PROBLEMS[name] = (m, n, p, S, A, B, sr.match(S[0], S[1], A, B, n, p))
    return _PROBLEMS[name]


def _device(pkg, ctx, name, dtype):
    """(S, A, {False: B, True: B^T}) on the device"""
    m, n, p, S, A, B, _ = _problem(name)
    return (_pattern_tiling(pkg, ctx, m, p, S, dtype), _tiling(pkg, ctx, m, n, A, dtype),
            {False: _tiling(pkg, ctx, n, p, B, dtype), True: _tiling(pkg, ctx, n, p, B, dtype, transposed=True)})


# ---- 1. against sampledref ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", NAMES)
def test_against_the_reference(pkg, oracle, tctx, name, dtype):
    m, n, p, S, A, B, matched = _problem(name)
    St, At, Bt = _device(pkg, tctx, name, dtype)
    for s in sr.SEMIRINGS:
        want = sr.fold(matched, A, B, s, dtype, oracle=oracle)
        for tb in (False, True):
            R = St.sampled_mxm(At, Bt[tb], s, transpose_b=tb)
            assert R.dtype == np.dtype(dtype) and (R.rows, R.cols, R.nnz) == (m, p, len(S[0]))
            assert _same(_vals(R), want, s), f"{name} {s} transpose_b={tb}"
    if name == "no_common_k":
        assert not np.any(np.diff(matched[0])), "every entry holds the start value"


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", sorted(sr.GENS) + ["rand_300", "dense_48", "band_1500", "rect_33x65_AAt", "empty_matrix"])
def test_four_tiles_per_wave_layout(pkg, oracle, tctx, monkeypatch, name, dtype):
    """PEM_SAMPLED_LPT=16, the measured alternative (16 lanes per pattern tile, sixteen accumulators per lane): the same bits, from
    the builder and from the accumulating refresh"""
    monkeypatch.setenv("PEM_SAMPLED_LPT", "16")
    m, n, p, S, A, B, matched = _problem(name)
    St, At, Bt = _device(pkg, tctx, name, dtype)
    for s in sr.SEMIRINGS:
        want = sr.fold(matched, A, B, s, dtype, oracle=oracle)
        for tb in (False, True):
            R = St.sampled_mxm(At, Bt[tb], s, transpose_b=tb)
            assert _same(_vals(R), want, s), f"{name} {s} transpose_b={tb}"
            if s in ("plus_times", "plus_pair", "lor_land"):
                R.set_values_sampled_mxm(At, Bt[tb], s, transpose_b=tb, accumulate=True)
                again = sr.fold(matched, A, B, s, dtype, old=want, oracle=oracle)
                assert _same(_vals(R), again, s), f"{name} {s} transpose_b={tb}: accumulate"


# ---- 2. against the masked plan on the GPU (consequences 1 and 2) -------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", NAMES)
def test_against_the_masked_plan(pkg, tctx, name, dtype):
    m, n, p, S, A, B, _ = _problem(name)
    St, At, Bt = _device(pkg, tctx, name, dtype)
    skeys = S[0] * p + S[1]
    for tb in (False, True):
        Bplan = Bt[True].transpose() if tb else Bt[False]   # the plan route needs a materialised B
        plan = pkg.CPlan(tctx, At, Bplan, mask=St)
        for s in sr.SEMIRINGS:
            plan.set_semiring(s)
            plan.spgemm()
            crp, cci, cv = plan.export_csr()
            R = St.sampled_mxm(At, Bt[tb], s, transpose_b=tb)
            got = _vals(R)
            stored = np.isin(skeys, sr.rows_of(crp) * p + cci)
            assert _same(got[stored], cv, s), f"{name} {s} transpose_b={tb}: where the plan stores an entry"
            start = np.full(int((~stored).sum()), sr.START[s], dtype)
            assert _same(got[~stored], start), f"{name} {s} transpose_b={tb}: the start value elsewhere"
            if s == "plus_pair":
                srp, sci, sv = R.select("value_ne", 0).export_csr()
                assert np.array_equal(srp, crp) and np.array_equal(sci, cci) and _same(sv, cv), f"{name} transpose_b={tb}: select(value_ne)"


# ---- 3. origins, aliases, special values --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", ("rand_300", "rect_33x65_AAt", "ragged"))
def test_other_value_type_and_transposed_origins(pkg, oracle, tctx, name, dtype):
    """an S of the other value type than A, and operands built with transpose = 1 (each is its own matrix)"""
    m, n, p, S, A, B, matched = _problem(name)
    other = np.float32 if dtype == np.float64 else np.float64
    So = _pattern_tiling(pkg, tctx, m, p, S, other)
    # from_coo(.., transpose=True) of the transposed triplets: the same matrices again
    ai, aj = sr.rows_of(A[0]).astype(np.int32), np.asarray(A[1], np.int32)
    bi, bj = sr.rows_of(B[0]).astype(np.int32), np.asarray(B[1], np.int32)
    At = pkg.Tiled.from_coo(tctx, n, m, aj, ai, A[2], True, dtype=dtype)
    Bt = {False: pkg.Tiled.from_coo(tctx, p, n, bj, bi, B[2], True, dtype=dtype),
          True: pkg.Tiled.from_coo(tctx, n, p, bi, bj, B[2], True, dtype=dtype)}
    assert (At.rows, At.cols) == (m, n) and (Bt[False].rows, Bt[False].cols) == (n, p) and (Bt[True].rows, Bt[True].cols) == (p, n)
    for s in sr.SEMIRINGS:
        want = sr.fold(matched, A, B, s, dtype, oracle=oracle)
        for tb in (False, True):
            R = So.sampled_mxm(At, Bt[tb], s, transpose_b=tb)
            assert R.dtype == np.dtype(dtype) and _same(_vals(R), want, s), f"{name} {s} transpose_b={tb}"


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", ("rand_300", "powerlaw_600", "dense_48"))
def test_one_handle(pkg, oracle, tctx, name, dtype):
    """S, A and B as one handle: A o (A * A) and A o (A * A^T)"""
    m, _, _, S, A, _, _ = _problem(name)
    T = _tiling(pkg, tctx, m, m, A, dtype)
    for tb in (False, True):
        B = sr.transpose(m, m, A) if tb else A
        matched = sr.match(S[0], S[1], A, B, m, m)
        for s in sr.SEMIRINGS:
            R = T.sampled_mxm(T, T, s, transpose_b=tb)
            assert _same(_vals(R), sr.fold(matched, A, B, s, dtype, oracle=oracle), s), f"{name} {s} transpose_b={tb}"


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", ("rand_50", "dense_48", "thin_tiles"))
def test_special_values(pkg, oracle, tctx, name, dtype):
    """+-0, +-inf, NaN and subnormals in A and B"""
    m, n, p, S, A, B, matched = _problem(name)
    rng = np.random.default_rng(11)
    A = (A[0], A[1], np.where(rng.random(len(A[2])) < 0.3, rng.choice(SPECIAL, len(A[2])), A[2]))
    B = (B[0], B[1], np.where(rng.random(len(B[2])) < 0.3, rng.choice(SPECIAL, len(B[2])), B[2]))
    St, At = _pattern_tiling(pkg, tctx, m, p, S, dtype), _tiling(pkg, tctx, m, n, A, dtype)
    Bt = {False: _tiling(pkg, tctx, n, p, B, dtype), True: _tiling(pkg, tctx, n, p, B, dtype, transposed=True)}
    for s in sr.SEMIRINGS:
        want = sr.fold(matched, A, B, s, dtype, oracle=oracle)
        for tb in (False, True):
            assert _same(_vals(St.sampled_mxm(At, Bt[tb], s, transpose_b=tb)), want, s), f"{name} {s} transpose_b={tb}"


# ---- 4. the new tiling against a from_csr rebuild -----------------------------------------------------------------------------------
def _assert_same_tiling(R, W, label, kind="plus_times"):
    for f in INFO:
        assert getattr(R, f) == getattr(W, f), f"{label}: info field {f}"
    for a in ARRAYS:
        x, y = R.array(a), W.array(a)
        assert (_same(x, y, kind) if a == "vals" else np.array_equal(x, y)), f"{label}: array {a}"


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", ("rand_300", "rect_70x40_AAt", "thin_tiles", "empty_sides", "empty_matrix"))
def test_result_equals_a_rebuild(pkg, oracle, tctx, name, dtype):
    """every pem_tiled_array and every info field but the timings"""
    m, n, p, S, A, B, matched = _problem(name)
    St, At, Bt = _device(pkg, tctx, name, dtype)
    rp, ci, _ = St.export_csr()
    for s, tb in (("plus_times", False), ("max_plus", True), ("plus_pair", False)):
        R = St.sampled_mxm(At, Bt[tb], s, transpose_b=tb)
        W = pkg.Tiled.from_csr(tctx, m, p, rp, ci, sr.fold(matched, A, B, s, dtype, oracle=oracle), dtype=dtype)
        _assert_same_tiling(R, W, f"{name} {s}", s)
    if name == "empty_matrix":
        assert (R.nnz, R.ntiles) == (0, 0)


# ---- 5. the refresh -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", ("rand_300", "rect_33x65_AAt", "band_1500", "long_lists"))
def test_refresh_after_new_operand_values(pkg, oracle, tctx, name, dtype):
    """after set_values_device on A the refresh equals a fresh build, in vals and in vals_t (read by the column walk of mxv)"""
    m, n, p, S, A, B, matched = _problem(name)
    St, At, Bt = _device(pkg, tctx, name, dtype)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    A2 = (A[0], A[1], np.random.default_rng(3).standard_normal(len(A[2])).astype(dtype))
    xv = torch.from_numpy(np.random.default_rng(4).standard_normal(m).astype(dtype)).cuda()
    for s in sr.SEMIRINGS:
        for tb in (False, True):
            R = St.sampled_mxm(At, Bt[tb], s, transpose_b=tb)
            At.set_values_device(torch.from_numpy(A2[2]).cuda())
            R.set_values(np.full(R.nnz, np.nan))   # poison both layouts
            R.set_values_sampled_mxm(At, Bt[tb], s, transpose_b=tb)
            W = St.sampled_mxm(At, Bt[tb], s, transpose_b=tb)
            assert _same(_vals(R), sr.fold(matched, A2, B, s, dtype, oracle=oracle), s), f"{name} {s} transpose_b={tb}"
            assert _same(R.array("vals"), W.array("vals"), s), f"{name} {s} transpose_b={tb}: vals against a fresh build"
            yt, wt = R.mxv(xv, transpose=True), W.mxv(xv, transpose=True)
            torch.cuda.synchronize()
            assert yt.dtype == tdt and _same(yt.cpu().numpy(), wt.cpu().numpy(), s), f"{name} {s} transpose_b={tb}: vals_t"
            At.set_values(A[2])


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", ("rand_300", "rect_33x65_AAt", "long_lists", "full_tile"))
def test_accumulate_splits_the_inner_dimension(pkg, tctx, name, dtype):
    """consequence 3: a call on (A1, B1) and an accumulate call on (A2, B2) equal one call on (A, B)"""
    m, n, p, S, A, B, _ = _problem(name)
    St, At, Bt = _device(pkg, tctx, name, dtype)
    for n1 in (1, 16, n // 2, n - 1):
        (A1, B1), (A2, B2) = sr.split_columns(A, B, n1, p)
        A1t, A2t = _tiling(pkg, tctx, m, n, A1, dtype), _tiling(pkg, tctx, m, n, A2, dtype)
        for tb in (False, True):
            B1t, B2t = _tiling(pkg, tctx, n, p, B1, dtype, transposed=tb), _tiling(pkg, tctx, n, p, B2, dtype, transposed=tb)
            for s in sr.SEMIRINGS:
                whole = _vals(St.sampled_mxm(At, Bt[tb], s, transpose_b=tb))
                R = St.sampled_mxm(A1t, B1t, s, transpose_b=tb)
                R.set_values_sampled_mxm(A2t, B2t, s, transpose_b=tb, accumulate=True)
                assert _same(_vals(R), whole, s), f"{name} {s} transpose_b={tb} n1={n1}"


def test_plans_turn_stale_repeat_calls_and_allocations(pkg, oracle, tctx):
    m, n, p, S, A, B, matched = _problem("band_1500")
    _, At, Bt = _device(pkg, tctx, "band_1500", np.float64)
    R = _pattern_tiling(pkg, tctx, m, p, S, np.float64)
    plan = pkg.CPlan(tctx, R, R)
    plan.spgemm()
    R.set_values_sampled_mxm(At, Bt[False])
    with pytest.raises(pkg.PemError) as e:
        plan.export_csr()
    assert e.value.status == PEM_E_STATE
    plan.step3()
    rp, ci, _ = R.export_csr()
    W = pkg.Tiled.from_csr(tctx, m, p, rp, ci, sr.fold(matched, A, B, "plus_times", np.float64, oracle=oracle))
    q = pkg.CPlan(tctx, W, W)
    q.spgemm()
    for x, y in zip(plan.export_csr(), q.export_csr()):
        assert _same(x, y), "step 3 after the refresh"
    # two calls give identical bits, and after the first refresh nothing is allocated
    for s in ("plus_times", "min_plus", "plus_pair"):
        for tb in (False, True):
            R.set_values_sampled_mxm(At, Bt[tb], s, transpose_b=tb)
            v1 = R.array("vals")
            tctx.synchronize()
            before = tctx.memory_stats()["block_allocs"]
            R.set_values_sampled_mxm(At, Bt[tb], s, transpose_b=tb)
            R.set_values_sampled_mxm(At, Bt[tb], s, transpose_b=tb, accumulate=True)
            R.set_values_sampled_mxm(At, Bt[tb], s, transpose_b=tb)
            tctx.synchronize()
            assert tctx.memory_stats()["block_allocs"] == before, f"{s} transpose_b={tb}: a repeat call allocated"
            assert np.array_equal(v1.view(np.uint64), R.array("vals").view(np.uint64)), f"{s} transpose_b={tb}: two calls differ"


# ---- 6. a hypersparse pattern ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_hypersparse(pkg, oracle, tctx, dtype):
    """more than 2^18 tile rows, tile columns and tiles: S = A, B = A^T, under plus_times and plus_pair"""
    n, I, J, V, _ = hypersparse()
    A = sr.csr(n, n, I, J, V)
    B = sr.transpose(n, n, A)
    SI = sr.rows_of(A[0])
    matched = sr.match(SI, A[1], A, B, n, n)
    T = pkg.Tiled.from_coo(tctx, n, n, I, J, V, dtype=dtype)
    Tt = T.transpose()
    for s in ("plus_times", "plus_pair"):
        want = sr.fold(matched, A, B, s, dtype, oracle=oracle)
        assert _same(_vals(T.sampled_mxm(T, T, s, transpose_b=True)), want, s), f"{s}: A * A^T from A's rows"
        assert _same(_vals(T.sampled_mxm(T, Tt, s, transpose_b=False)), want, s), f"{s}: A * A^T from the transpose's columns"


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments(pkg, tctx):
    L = pkg.lib()
    m, n, p, S, A, B, _ = _problem("ragged")
    St, At, Bt = _device(pkg, tctx, "ragged", np.float64)
    Sf, Af, Bf = _device(pkg, tctx, "ragged", np.float32)
    R = St.sampled_mxm(At, Bt[False])

    def build(ctx=tctx._h, s=St._h, a=At._h, b=Bt[False]._h, tb=0, sem=0, out=True):
        h = C.c_void_p(0xdead)
        st = L.pem_tiled_sampled_mxm(ctx, s, a, b, tb, sem, C.byref(h) if out else None)
        if st == 0:
            assert L.pem_tiled_destroy(ctx, h) == 0
        elif out:
            assert not h.value, "*out stays NULL"
        return st

    def inplace(ctx=tctx._h, t=R._h, a=At._h, b=Bt[False]._h, tb=0, sem=0, acc=0):
        return L.pem_tiled_set_values_sampled_mxm(ctx, t, a, b, tb, sem, acc)

    assert build() == 0 and build(b=Bt[True]._h, tb=1) == 0 and inplace() == 0 and inplace(b=Bt[True]._h, tb=1, acc=1) == 0
    version = R.array("vals")
    bad = [build(ctx=None), build(s=None), build(a=None), build(b=None), build(out=False), build(sem=6), build(sem=-1), build(tb=2),
           build(tb=-1), build(a=Af._h), build(b=Bf[False]._h),                    # A and B of different value types
           build(b=Bt[True]._h), build(b=Bt[False]._h, tb=1),                      # inner dimensions (53 against 29)
           build(s=At._h), build(s=Bt[False]._h),                                  # a pattern that is not m x p
           inplace(ctx=None), inplace(t=None), inplace(a=None), inplace(b=None), inplace(sem=6), inplace(sem=-1), inplace(tb=2),
           inplace(acc=2), inplace(acc=-1), inplace(a=Af._h), inplace(b=Bf[False]._h),
           inplace(a=Af._h, b=Bf[False]._h),                                       # t of another value type than A
           inplace(b=Bt[True]._h), inplace(t=At._h)]                               # inner dimensions; not m x p (and t == A)
    assert bad == [PEM_E_INVALID] * len(bad)
    assert b"pem_tiled_set_values_sampled_mxm" in L.pem_last_error()
    # t == A and t == B on shapes that would pass: a square tiling
    _, Qa, Qb = _device(pkg, tctx, "rand_50", np.float64)
    Q2 = _device(pkg, tctx, "rand_50", np.float64)[1]
    assert inplace(t=Qa._h, a=Qa._h, b=Q2._h) == PEM_E_INVALID and inplace(t=Qa._h, a=Q2._h, b=Qa._h) == PEM_E_INVALID
    assert inplace(t=Qa._h, a=Q2._h, b=Q2._h) == 0
    tctx.synchronize()
    assert np.array_equal(version.view(np.uint64), R.array("vals").view(np.uint64)), "a refused call wrote nothing"
    # an S of the other value type is fine for the builder; the Python layer
    assert build(s=Sf._h) == 0
    with pytest.raises(ValueError):
        St.sampled_mxm(At, Bt[False], "plus_min")
    with pytest.raises(ValueError):
        R.set_values_sampled_mxm(At, Bt[False], "plus_min")


# ---- 8. triangle counting -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_triangle_count(pkg, tctx, dtype):
    P = sr.CASES["powerlaw_600"]
    for n, I, J in (sr.triangle_graph(), (600,) + sr.symmetrised(600, P[2], P[3])):
        A = pkg.Tiled.from_coo(tctx, n, n, I, J, np.full(len(I), 0.5), dtype=dtype)
        got = pkg.triangle_count(A)
        assert isinstance(got, int) and got == sr.triangles(n, I, J) and got > 0
