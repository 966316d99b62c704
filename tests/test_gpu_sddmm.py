"""GPU: the sampled dense-dense product of a tiling (pem_tiled_sddmm / pem_tiled_set_values_sddmm).

Every comparison is bit for bit over every entry (NaN == NaN; +0 == -0 under min / max only): there is no tolerance and no entry
is left out.  The references: sddmmref (the oracle's fma chain per entry, numpy folds for the other semirings), the plan route on
the GPU (X and Y^T as dense tilings, a plan masked by the pattern), and a from_csr rebuild with the reference values.

Cases left out of the sddmmref sweep (test_against_the_reference): k64_bins and wide_tilecols.  X has rows x k elements whatever the
entry count, and with 2.1 M and 262 k rows the dense host operands of a 14-k sweep in six semirings, not the O(nnz * k) reference,
are what costs; both run against the plan route at k = 5 with the other BIG cases of test_gpu_spmm.py.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import mxvref as mr
import sddmmref as sd
import spmmref as spr
from matgen import cases

pytestmark = pytest.mark.gpu

torch.cuda.is_available()   # (torch's runtime first, as in the other GPU files)

CASES = cases()
PEM_E_INVALID, PEM_E_STATE = -1, -6
DTYPES = (np.float64, np.float32)
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3.0e-310, 1.0e-40, 0.5, -0.5, 2.0])
MINMAX = ("min_plus", "max_plus", "max_times")
# the kernel compiles the chunk widths 4, 8 and 16 (the narrowest that holds k; 16 and several chunks past that): 0, then W - 1, W,
# W + 1 for each width, two chunks, two chunks + 1, and 40 = 16 + 16 + 8 (three chunks, the last one partial)
KS = (0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 32, 33, 40)
BIG = ("wide_tilecols", "k64_bins", "hub_tile_2100_AAt", "blockrows_10000")
NO_SWEEP = ("wide_tilecols", "k64_bins")
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


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _same(got, want, kind="plus_times"):
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    ok = (got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want))
    if kind in MINMAX:
        ok |= (got == 0) & (want == 0)
    return bool(np.all(ok))


def _specials(shape, seed, dtype):
    """values with about a quarter replaced by +-0, +-inf, NaN and subnormals"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(shape)
    sp = rng.random(v.shape) < 0.25
    v[sp] = rng.choice(SPECIAL, int(sp.sum()))
    return v.astype(dtype)


def _tiled(pkg, ctx, case, dtype, transpose=False):
    rows, cols, I, J, V, _ = case
    return pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, transpose, dtype=dtype)


def _pattern(T):
    """(rowptr, colidx, I, J) of a tiling, entries in CSR order"""
    rp, ci, _ = T.export_csr()
    I, J = sd.pattern_of(T.rows, rp, ci)
    return rp, ci, I, J


def _operands(S, k, seed, dtype):
    """X (rows x k) and Y (cols x k) as column slices of wider buffers with different row strides, host and device"""
    Xw, Yw = _specials((S.rows, k + 3), seed, dtype), _specials((S.cols, k + 11), seed + 1, dtype)
    Xd, Yd = _dev(Xw), _dev(Yw)
    return Xw[:, 2:2 + k], Yw[:, 5:5 + k], Xd[:, 2:2 + k], Yd[:, 5:5 + k]


def _vals(T):
    return T.export_csr()[2]


def _rebuild(pkg, ctx, rows, cols, rp, ci, vals, dtype):
    return pkg.Tiled.from_csr(ctx, rows, cols, rp, ci, vals, dtype=dtype)


def _assert_same_tiling(R, W, label, kind="plus_times"):
    for f in INFO:
        assert getattr(R, f) == getattr(W, f), f"{label}: info field {f}"
    for a in ARRAYS:
        x, y = R.array(a), W.array(a)
        assert (_same(x, y, kind) if a == "vals" else np.array_equal(x, y)), f"{label}: array {a}"


# ---- 1. against sddmmref ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", sorted(n for n in CASES if n not in NO_SWEEP))
def test_against_the_reference(pkg, oracle, tctx, name, dtype):
    S = _tiled(pkg, tctx, CASES[name], np.float64)   # (the builder takes an S of either value type: here fp64 for both)
    _, _, I, J = _pattern(S)
    kmax = max(KS)
    Xh, Yh, X, Y = _operands(S, kmax, 100, dtype)
    for s in sd.SEMIRINGS:
        R = None
        for k in KS:
            want = sd.sddmm(I, J, Xh[:, :k], Yh[:, :k], s, dtype, oracle=oracle)
            R = S.sddmm(X[:, :k], Y[:, :k], s)
            assert R.dtype == np.dtype(dtype) and (R.rows, R.cols, R.nnz) == (S.rows, S.cols, S.nnz)
            assert _same(_vals(R), want, s), f"{name} {s} k={k}"
        # accumulate: the columns [5, 5 + k2) on top of what the tiling holds (its own bits, so zero signs under min / max agree)
        for k2 in (4, 17):
            old = _vals(R)
            want = sd.sddmm(I, J, Xh[:, 5:5 + k2], Yh[:, 5:5 + k2], s, dtype, old=old, oracle=oracle)
            R.set_values_sddmm(X[:, 5:5 + k2], Y[:, 5:5 + k2], s, accumulate=True)
            assert _same(_vals(R), want, s), f"{name} {s} accumulate k={k2}"


# ---- 2. against the plan route ------------------------------------------------------------------------------------------------------
def _plan_route(pkg, ctx, S, Xh, Yh, s, dtype):
    """C<S> = Xt * Ytt under s: Xt the dense rows x k tiling of X, Ytt the dense k x cols tiling of Y^T"""
    k = Xh.shape[1]
    ii, cc = np.meshgrid(np.arange(S.rows, dtype=np.int32), np.arange(k, dtype=np.int32), indexing="ij")
    jj, c2 = np.meshgrid(np.arange(S.cols, dtype=np.int32), np.arange(k, dtype=np.int32), indexing="ij")
    Xt = pkg.Tiled.from_coo(ctx, S.rows, k, ii.ravel(), cc.ravel(), np.ascontiguousarray(Xh).ravel(), dtype=dtype)
    Ytt = pkg.Tiled.from_coo(ctx, k, S.cols, c2.ravel(), jj.ravel(), np.ascontiguousarray(Yh).ravel(), dtype=dtype)
    p = pkg.CPlan(ctx, Xt, Ytt, mask=S, semiring=s)
    p.spgemm()
    return p.export_csr()


def _check_plan_route(pkg, tctx, name, k, dtype):
    S = _tiled(pkg, tctx, CASES[name], dtype)
    rp, ci, _, _ = _pattern(S)
    Xh, Yh, X, Y = _operands(S, k, 200 + k, dtype)
    for s in sd.SEMIRINGS:
        R = S.sddmm(X, Y, s)
        crp, cci, cv = _plan_route(pkg, tctx, S, Xh, Yh, s, dtype)
        assert np.array_equal(crp, rp) and np.array_equal(cci, ci), f"{name} {s} k={k}: the masked plan's pattern is not S's"
        assert _same(_vals(R), cv, s), f"{name} {s} k={k}"


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("k", (1, 5, 16))
@pytest.mark.parametrize("name", ("tiny_9x9", "rand_300", "rect_70x40_AAt", "rect_33x65_AAt", "empty_rows", "dense_48", "powerlaw_600",
                                  "band_1500", "hub_row_4000"))
def test_plan_route(pkg, tctx, name, k, dtype):
    _check_plan_route(pkg, tctx, name, k, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", BIG)
def test_plan_route_big(pkg, tctx, name, dtype):
    """the cases the O(nnz * k) reference and its dense host operands do not reach, at k = 5"""
    _check_plan_route(pkg, tctx, name, 5, dtype)


# ---- 3. the new tiling against a from_csr rebuild ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", ("rand_300", "rect_70x40_AAt", "powerlaw_600", "dense_tile"))
def test_result_equals_a_rebuild_from_every_origin(pkg, oracle, tctx, tmp_path, name, dtype):
    """every pem_tiled_array and every info field but the timings; S of the other value type, S built with transpose = 1, S from
    from_cplan, ewise, select and load"""
    other = np.float32 if dtype == np.float64 else np.float64
    A = _tiled(pkg, tctx, CASES[name], dtype)
    At = _tiled(pkg, tctx, CASES[name], dtype, transpose=True)
    assert (At.rows, At.cols) == (A.cols, A.rows)
    p = pkg.CPlan(tctx, A, At)
    p.spgemm()
    path = str(tmp_path / "a.pemt")
    A.save(path)
    origins = {"converted": A, "other value type": _tiled(pkg, tctx, CASES[name], other), "transposed": At,
               "from_cplan": pkg.Tiled.from_cplan(p), "from_cplan^T": pkg.Tiled.from_cplan(p, transpose=True),
               "ewise": pkg.Tiled.ewise(A, A, "max"), "select": A.select("tril", 0), "loaded": pkg.Tiled.load(tctx, path)}
    for label, S in origins.items():
        rp, ci, I, J = _pattern(S)
        for k, s in ((5, "plus_times"), (17, "max_plus"), (0, "min_plus")):
            Xh, Yh, X, Y = _operands(S, k, 300 + k, dtype)
            R = S.sddmm(X, Y, s)
            W = _rebuild(pkg, tctx, S.rows, S.cols, rp, ci, sd.sddmm(I, J, Xh, Yh, s, dtype, oracle=oracle), dtype)
            _assert_same_tiling(R, W, f"{name} {label} {s} k={k}", s)


# ---- 4. in place --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", ("rand_300", "rect_70x40_AAt", "band_1500", "blockrows_1600"))
def test_in_place_writes_both_value_layouts(pkg, oracle, tctx, name, dtype):
    """vals against a rebuild; vals_t through its readers: R as the B operand of a plan and R.mxv(transpose=True)"""
    R = _tiled(pkg, tctx, CASES[name], dtype)
    rp, ci, I, J = _pattern(R)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    Ah = _specials((40, R.rows), 7, dtype)
    ii, jj = np.meshgrid(np.arange(40, dtype=np.int32), np.arange(R.rows, dtype=np.int32), indexing="ij")
    A0 = pkg.Tiled.from_coo(tctx, 40, R.rows, ii.ravel(), jj.ravel(), Ah.ravel(), dtype=dtype)
    xv = _dev(_specials(R.rows, 8, dtype))
    for k, s in ((5, "plus_times"), (16, "plus_times"), (33, "max_times"), (9, "lor_land")):
        Xh, Yh, X, Y = _operands(R, k, 400 + k, dtype)
        R.set_values(np.full(R.nnz, np.nan))   # poison both layouts
        R.set_values_sddmm(X, Y, s)
        W = _rebuild(pkg, tctx, R.rows, R.cols, rp, ci, sd.sddmm(I, J, Xh, Yh, s, dtype, oracle=oracle), dtype)
        assert _same(R.array("vals"), W.array("vals"), s), f"{name} {s} k={k}: vals"
        got, want = pkg.CPlan(tctx, A0, R), pkg.CPlan(tctx, A0, W)
        got.spgemm()
        want.spgemm()
        for x, y in zip(got.export_csr(), want.export_csr()):
            assert _same(x, y, s), f"{name} {s} k={k}: vals_t as the B operand of a plan"
        yt, wt = R.mxv(xv, transpose=True), W.mxv(xv, transpose=True)
        assert yt.dtype == tdt and _same(_host(yt), _host(wt), s), f"{name} {s} k={k}: vals_t under the column walk"


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", ("rand_300", "powerlaw_600", "dense_48"))
def test_accumulate_splits_the_columns_and_x_is_y(pkg, oracle, tctx, name, dtype):
    R = _tiled(pkg, tctx, CASES[name], dtype)
    _, _, I, J = _pattern(R)
    assert R.rows == R.cols
    for k1, k2 in ((3, 4), (16, 21), (0, 5), (5, 0)):
        Xh, Yh, X, Y = _operands(R, k1 + k2, 500 + k1, dtype)
        for s in sd.SEMIRINGS:
            R.set_values_sddmm(X, Y, s)
            whole = _vals(R)
            assert _same(whole, sd.sddmm(I, J, Xh, Yh, s, dtype, oracle=oracle), s), f"{name} {s} k={k1 + k2}"
            R.set_values_sddmm(X[:, :k1], Y[:, :k1], s)
            R.set_values_sddmm(X[:, k1:], Y[:, k1:], s, accumulate=True)
            assert _same(_vals(R), whole, s), f"{name} {s}: {k1} + {k2} columns"
            # X is Y: the same pointer, and Y=None
            R.set_values_sddmm(X, X, s)
            same_ptr = _vals(R)
            assert _same(same_ptr, sd.sddmm(I, J, Xh, Xh, s, dtype, oracle=oracle), s), f"{name} {s}: X is Y"
            R.set_values_sddmm(X, None, s)
            assert _same(_vals(R), same_ptr), f"{name} {s}: Y=None"
            assert _same(_vals(R.sddmm(X, semiring=s)), same_ptr), f"{name} {s}: sddmm(X)"


def test_plans_turn_stale_repeat_calls_and_allocations(pkg, oracle, tctx):
    case = CASES["band_1500"]
    R = _tiled(pkg, tctx, case, np.float64)
    rp, ci, I, J = _pattern(R)
    p = pkg.CPlan(tctx, R, R)
    p.spgemm()
    Xh, Yh, X, Y = _operands(R, 12, 600, np.float64)
    R.set_values_sddmm(X, Y)
    with pytest.raises(pkg.PemError) as e:
        p.export_csr()
    assert e.value.status == PEM_E_STATE
    p.step3()
    W = _rebuild(pkg, tctx, R.rows, R.cols, rp, ci, sd.sddmm(I, J, Xh, Yh, "plus_times", np.float64, oracle=oracle), np.float64)
    q = pkg.CPlan(tctx, W, W)
    q.spgemm()
    for x, y in zip(p.export_csr(), q.export_csr()):
        assert _same(x, y), "step 3 after the refresh"
    # two calls give identical bits, and the second allocates nothing
    for k in (3, 40):
        H = _dev(_specials((R.rows, k), 9, np.float64))
        for s in ("plus_times", "min_plus", "plus_pair"):
            R.set_values_sddmm(H, None, s)
            v1 = R.array("vals")
            tctx.synchronize()
            before = tctx.memory_stats()["block_allocs"]
            R.set_values_sddmm(H, None, s)
            tctx.synchronize()
            assert tctx.memory_stats()["block_allocs"] == before, f"{s} k={k}: a repeat call allocated"
            assert np.array_equal(v1.view(np.uint64), R.array("vals").view(np.uint64)), f"{s} k={k}: two calls differ"


def test_graph_replay_survives_a_refresh(pkg, oracle, ctx):
    case = CASES["band_1500"]
    g = pkg.Context(0)
    try:
        g.set_graph_replay(True)
        R = _tiled(pkg, g, case, np.float64)
        rp, ci, I, J = _pattern(R)
        plan = pkg.CPlan(g, R, R)
        plan.spgemm()
        plan.spgemm()   # repeat pass: captured and replayed
        plan.spgemm()
        for seed in (2, 3, 4):
            Xh = _specials((R.rows, 6), seed, np.float64)
            H = _dev(Xh)
            R.set_values_sddmm(H)
            g.synchronize()
            plan.spgemm()
            W = _rebuild(pkg, ctx, R.rows, R.cols, rp, ci, sd.sddmm(I, J, Xh, Xh, "plus_times", np.float64, oracle=oracle), np.float64)
            fresh = pkg.CPlan(ctx, W, W)
            fresh.spgemm()
            for x, y in zip(plan.export_csr(), fresh.export_csr()):
                assert _same(x, y), seed
    finally:
        g.close()


# ---- 5. downstream ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_result_feeds_spmm_and_reduce(pkg, oracle, tctx, dtype):
    """the attention pair R = S.sddmm(Q, K); O = R.spmm(V), and the row sums of R"""
    S = _tiled(pkg, tctx, CASES["powerlaw_600"], dtype)
    rp, ci, I, J = _pattern(S)
    rng = np.random.default_rng(3)
    Qh, Kh, Vh = (rng.standard_normal((S.rows, 8)).astype(dtype), rng.standard_normal((S.cols, 8)).astype(dtype),
                  rng.standard_normal((S.cols, 6)).astype(dtype))
    R = S.sddmm(_dev(Qh), _dev(Kh))
    rv = sd.sddmm(I, J, Qh, Kh, "plus_times", dtype, oracle=oracle)
    assert _same(_vals(R), rv)
    O = R.spmm(_dev(Vh))
    assert _same(_host(O), spr.spmm(S.rows, S.cols, rp, ci, rv, Vh, "plus_times", dtype, oracle=oracle))
    assert _same(_host(R.reduce("plus", "rows")), mr.reduce(S.rows, S.cols, rp, ci, rv, "plus", dtype))


def test_empty_tiling(pkg, tctx):
    E = _tiled(pkg, tctx, CASES["empty_matrix"], np.float64)
    X = _dev(np.ones((E.rows, 3)))
    for s in sd.SEMIRINGS:
        R = E.sddmm(X, semiring=s)
        assert (R.nnz, R.ntiles) == (0, 0)
        _assert_same_tiling(R, E, f"empty {s}")
        E.set_values_sddmm(X, semiring=s, accumulate=True)
    assert R.export_csr()[0].tolist() == [0] * (E.rows + 1)


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments(pkg, tctx):
    L = pkg.lib()
    case = CASES["rect_70x40_AAt"]
    rows, cols = case[0], case[1]
    A, F = _tiled(pkg, tctx, case, np.float64), _tiled(pkg, tctx, case, np.float32)
    k = 5
    X, Y = _dev(np.ones((rows, k))), _dev(np.ones((cols, k)))
    XF, YF = _dev(np.ones((rows, k), np.float32)), _dev(np.ones((cols, k), np.float32))
    px, py = C.c_void_p(X.data_ptr()), C.c_void_p(Y.data_ptr())
    i64 = C.c_int64

    def inplace(ctx=tctx._h, T=A._h, s=0, kk=k, x=px, ldx=k, y=py, ldy=k, acc=0, fn=L.pem_tiled_set_values_sddmm):
        return fn(ctx, T, s, i64(kk), x, i64(ldx), y, i64(ldy), acc)

    def build(ctx=tctx._h, T=A._h, s=0, kk=k, x=px, ldx=k, y=py, ldy=k, out=True, fn=L.pem_tiled_sddmm):
        h = C.c_void_p()
        st = fn(ctx, T, s, i64(kk), x, i64(ldx), y, i64(ldy), C.byref(h) if out else None)
        if st == 0:
            assert L.pem_tiled_destroy(ctx, h) == 0
        else:
            assert not h.value
        return st

    assert inplace() == 0 and build() == 0
    bad = [inplace(ctx=None), inplace(T=None), inplace(s=6), inplace(s=-1), inplace(acc=2), inplace(acc=-1), inplace(kk=-1),
           inplace(ldx=k - 1), inplace(ldy=k - 1), inplace(kk=0, ldx=0), inplace(kk=0, ldy=0), inplace(x=None), inplace(y=None),
           inplace(ldx=2 ** 62), inplace(ldy=2 ** 62),
           inplace(fn=L.pem_tiled_set_values_sddmm_f32, x=C.c_void_p(XF.data_ptr()), y=C.c_void_p(YF.data_ptr())),   # fp64 tiling, fp32 entry
           inplace(T=F._h),                                                                                          # fp32 tiling, fp64 entry
           build(ctx=None), build(T=None), build(out=False), build(s=6), build(kk=-1), build(ldx=k - 1), build(ldy=k - 1), build(x=None),
           build(y=None), build(ldx=2 ** 62), build(ldy=2 ** 62)]
    assert bad == [PEM_E_INVALID] * len(bad)
    assert b"pem_tiled_sddmm" in L.pem_last_error()
    # null pointers are fine where nothing is read: k = 0, and plus_pair
    assert inplace(kk=0, x=None, y=None, ldx=1, ldy=1) == 0 and build(kk=0, x=None, y=None, ldx=1, ldy=1) == 0
    assert inplace(s=4, x=None, y=None) == 0 and build(s=4, x=None, y=None) == 0
    # the builder takes an S of the other value type
    assert build(T=F._h) == 0 and build(fn=L.pem_tiled_sddmm_f32, x=C.c_void_p(XF.data_ptr()), y=C.c_void_p(YF.data_ptr())) == 0
    tctx.synchronize()
    # the Python layer
    for bad_x in (_dev(np.ones(rows)), _dev(np.ones((k, rows))).t(), np.ones((rows, k)), _dev(np.ones((rows + 1, k))),
                  torch.ones((rows, k), dtype=torch.float64), _dev(np.ones((rows, k), np.float16))):
        with pytest.raises(ValueError, match="want a 2-D device tensor"):
            A.sddmm(bad_x, Y)
    for call in (lambda: A.sddmm(X, _dev(np.ones((cols, k + 1)))), lambda: A.sddmm(X, YF), lambda: A.sddmm(X, _dev(np.ones((cols + 1, k)))),
                 lambda: A.set_values_sddmm(XF, YF), lambda: F.set_values_sddmm(X, Y), lambda: A.set_values_sddmm(X, Y.t().contiguous().t())):
        with pytest.raises(ValueError, match="want a 2-D device tensor"):
            call()
    with pytest.raises(ValueError, match="square"):
        A.sddmm(X)
    with pytest.raises(ValueError):
        A.sddmm(X, Y, "plus_min")
    with pytest.raises(ValueError):
        A.set_values_sddmm(X, Y, "plus_min")
    assert F.sddmm(X, Y).dtype == np.float64 and A.sddmm(XF, YF).dtype == np.float32   # R's dtype is X's
