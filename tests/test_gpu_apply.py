"""GPU: apply and scale (pem_tiled_apply, pem_tiled_scale) and their refreshes (pem_tiled_set_values_from_apply / _scale).

The central check: the tiling made on the device equals, array for array, the tiling pem_tiled_from_coo builds from the same entries
with applyref's values -- every pem_tiled_info field but the timings, all twelve arrays, values bit for bit (NaN equals NaN; zeros
may differ in sign for min / max).  vals_t is no pem_tiled_array: it is checked through its readers, mxv(transpose=True) and step 3's
B side.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import applyref as ap
from matgen import cases, hypersparse

pytestmark = pytest.mark.gpu

torch.cuda.is_available()   # (torch's runtime first, as in the other GPU files)

CASES = cases()
PEM_E_INVALID = -1
DTYPES = (np.float64, np.float32)
IDS = ("f64", "f32")
INFO = ("rows", "cols", "nnz", "tile_rows", "tile_cols", "ntiles", "value_bytes")
ARRAYS = ("tile_keys", "tile_nnz_ptr", "masks", "rowptr", "rowcolidx", "vals", "masks_t", "tile_rowptr", "tile_colidx", "tile_colptr",
          "tile_rowidx", "tile_offsets")
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3.0e-310, 1.0e-40, 0.5, -0.5])
SMALL = ("one_entry", "tiny_9x9", "ragged_37", "dense_tile", "dense_48", "empty_matrix", "empty_rows", "rect_33x65_AAt", "row_vector_AAt",
         "col_vector_AAt", "cancel_and_zero", "rand_300", "powerlaw_600")
LARGE = ("hub_row_4000", "wide_tilecols", "blockrows_1600")
# every op with the thunks it is run with: unary ops ignore theirs
THUNKS = {op: (0.0,) for op in ap.UNARY}
THUNKS.update({op: (0.25, -3.0) for op in ("plus", "times", "min", "max", "div", "rdiv", "rminus")})
THUNKS["div"] = (0.25, 3.0, 0.0)
THUNKS["rdiv"] = (1.0, -3.0)
THUNKS["times"] = (0.1, np.inf)
THUNKS["powi"] = (1, 2, 3, 7, 64)


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


def _same_results(xs, ys, op="plus"):
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


def _case(name, dtype, transpose=False):
    """(rows, cols, I, J, V) of the matrix the tiling represents, canonical, values with specials in the dtype"""
    rows, cols, I, J, V, _ = CASES[name]
    rng = np.random.default_rng(3 + rows * 7 + cols)
    Vd = _specials(rng, V).astype(dtype)
    if transpose:
        rows, cols, I, J = cols, rows, J, I
    return (rows, cols) + _canonical(I, J, Vd, cols)


def _vectors(rows, cols, dtype, seed=11, special=True):
    rng = np.random.default_rng(seed + rows + 3 * cols)
    r, c = rng.normal(size=rows), rng.normal(size=cols)
    if special:
        r, c = _specials(rng, r), _specials(rng, c)
    return r.astype(dtype), c.astype(dtype)


def _dev(*arrays):
    out = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]
    torch.cuda.synchronize()   # (the vectors are read on the context's stream)
    return out


def _scaled(pkg, A, r, c, op):
    dr, dc = _dev(r, c)
    R = A.scale(dr, dc, op)
    return R


VEC_MODES = ("rows", "cols", "both", "neither")


def _pick(mode, r, c):
    return (r if mode in ("rows", "both") else None), (c if mode in ("cols", "both") else None)


# ---- equality with applyref + from_coo ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", SMALL)
def test_every_apply_op(pkg, ctx, name, dtype):
    rows, cols, I, J, V = _case(name, dtype)
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=dtype)
    for op in ap.OPS:
        for thunk in THUNKS[op]:
            R = A.apply(op, thunk)
            want = pkg.Tiled.from_coo(ctx, rows, cols, I, J, ap.apply(V, op, thunk, dtype), dtype=dtype)
            _assert_same_tiling(R, want, f"{name} {op}:{thunk}", op)
    _assert_same_tiling(A.apply("identity"), A, f"{name} identity is a copy")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", LARGE)
def test_apply_and_scale_on_the_large_cases(pkg, ctx, name, dtype):
    """tile counts across several 64-tile chunks, 16 385 tile rows, a hub row"""
    rows, cols, I, J, V = _case(name, dtype)
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=dtype)
    for op, thunk in (("minv", 0.0), ("powi", 5)):
        want = pkg.Tiled.from_coo(ctx, rows, cols, I, J, ap.apply(V, op, thunk, dtype), dtype=dtype)
        _assert_same_tiling(A.apply(op, thunk), want, f"{name} {op}")
    r, c = _vectors(rows, cols, dtype)
    for op in ("times", "plus"):
        want = pkg.Tiled.from_coo(ctx, rows, cols, I, J, ap.scale(I, J, V, r, c, op, dtype), dtype=dtype)
        _assert_same_tiling(_scaled(pkg, A, r, c, op), want, f"{name} scale {op}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", SMALL)
def test_every_scale_op_and_vector_combination(pkg, ctx, name, dtype):
    rows, cols, I, J, V = _case(name, dtype)
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=dtype)
    r, c = _vectors(rows, cols, dtype)       # exactly rows / cols long: a read past the end of either is a read out of bounds
    dr, dc = _dev(r, c)
    for op in ap.BINOPS:
        for mode in VEC_MODES:
            (hr, hc), (tr, tc) = _pick(mode, r, c), _pick(mode, dr, dc)
            R = A.scale(tr, tc, op)
            want = pkg.Tiled.from_coo(ctx, rows, cols, I, J, ap.scale(I, J, V, hr, hc, op, dtype), dtype=dtype)
            _assert_same_tiling(R, want, f"{name} scale {op} {mode}", op)
            if mode == "neither":
                assert np.array_equal(_bits(R.array("vals")), _bits(A.array("vals"))), "no vector: the values are A's bit for bit"


# ---- vals_t, through its readers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ("rand_300", "rect_33x65_AAt", "ragged_37", "dense_48", "powerlaw_600", "blockrows_1600"))
def test_vals_t_through_its_readers(pkg, ctx, name, dtype):
    rows, cols, I, J, V = _case(name, dtype)
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=dtype)
    r, c = _vectors(rows, cols, dtype)
    x, = _dev(np.random.default_rng(5).normal(size=rows).astype(dtype))
    X = pkg.Tiled.from_coo(ctx, cols, rows, J, I, np.asarray(V), dtype=dtype)            # cols x rows: the A side of X * R
    made = [(A.apply(op, th), ap.apply(V, op, th, dtype), f"apply {op}", op) for op, th in (("rdiv", 2.0), ("abs", 0), ("powi", 3), ("one", 0))]
    made += [(_scaled(pkg, A, hr, hc, op), ap.scale(I, J, V, hr, hc, op, dtype), f"scale {op}", op)
             for op, (hr, hc) in (("times", (r, c)), ("plus", (r, None)), ("max", (None, c)), ("lor", (r, c)))]
    for R, Vw, label, op in made:                               # (after max the sign of a zero is free, and a product inherits it)
        want = pkg.Tiled.from_coo(ctx, rows, cols, I, J, Vw, dtype=dtype)
        for sr in ("plus_times", "min_plus"):
            got_y, want_y = R.mxv(x, sr, transpose=True), want.mxv(x, sr, transpose=True)
            ctx.synchronize()
            assert _same_vals(got_y.cpu().numpy(), want_y.cpu().numpy(), op), f"{name} {label}: mxv^T under {sr}"
            pg, pw = pkg.CPlan(ctx, X, R, semiring=sr), pkg.CPlan(ctx, X, want, semiring=sr)
            pg.spgemm()
            pw.spgemm()
            assert _same_results(pg.export_csr(), pw.export_csr(), op), f"{name} {label}: R as B under {sr}"


# ---- an independent route: products with diagonal tilings ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ("rand_300", "rect_33x65_AAt", "ragged_37", "powerlaw_600"))
def test_scale_equals_products_with_diagonal_tilings(pkg, ctx, name, dtype):
    """D_r * A * D_c through two plans and from_cplan: under plus_times fma(r, a, 0) is the product rounded once (only the sign of a
    zero may differ), under min_plus min(inf, r + a) is the sum.  Values and vectors are finite here (zeros and subnormals among
    them): a NaN is skipped by min_plus but kept by scale, which is the documented difference, not the subject."""
    rows, cols, I, J, _ = _case(name, dtype)
    rng = np.random.default_rng(17)
    fin = np.array([0.0, -0.0, 3.0e-310, 1.0e-40, 0.5, -0.5, 1.0e30])
    mix = lambda n: np.where(rng.random(n) < 0.2, rng.choice(fin, n), rng.normal(size=n)).astype(dtype)
    V, r, c = mix(len(I)), mix(rows), mix(cols)
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=dtype)
    Dr = pkg.Tiled.from_coo(ctx, rows, rows, np.arange(rows), np.arange(rows), r, dtype=dtype)
    Dc = pkg.Tiled.from_coo(ctx, cols, cols, np.arange(cols), np.arange(cols), c, dtype=dtype)
    for op, sr in (("times", "plus_times"), ("plus", "min_plus")):
        p1 = pkg.CPlan(ctx, Dr, A, semiring=sr)
        p1.spgemm()
        p2 = pkg.CPlan(ctx, pkg.Tiled.from_cplan(p1), Dc, semiring=sr)
        p2.spgemm()
        want = pkg.Tiled.from_cplan(p2)
        got = _scaled(pkg, A, r, c, op)
        for k in INFO:
            assert getattr(got, k) == getattr(want, k), f"{name} {op}: {k}"
        for arr in ARRAYS:
            g, w = got.array(arr), want.array(arr)
            if arr == "vals":
                assert np.all((_bits(g) == _bits(w)) | ((g == 0) & (w == 0)) | (np.isnan(g) & np.isnan(w))), f"{name} {op}: values"
            else:
                assert np.array_equal(g, w), f"{name} {op}: array {arr}"


# ---- refresh -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_apply_refresh_equals_fresh_and_allocates_nothing(pkg, ctx, dtype):
    rows, cols, I, J, V = _case("powerlaw_600", dtype)
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=dtype)
    rng = np.random.default_rng(41)
    state = {v: k for k, v in pkg.STATUS_NAMES.items()}["PEM_E_STATE"]
    for op, thunk in (("abs", 0), ("minv", 0), ("times", 0.3), ("powi", 3), ("one", 0), ("identity", 0)):
        R = A.apply(op, thunk)
        down = pkg.CPlan(ctx, A, R)                              # reads R's vals_t
        down.spgemm()
        for _ in range(2):
            A.set_values(_specials(rng, rng.normal(size=A.nnz)))
            before = ctx.memory_stats()["block_allocs"]
            R.set_values_from_apply(A)                          # (the very first call allocates nothing either)
            assert ctx.memory_stats()["block_allocs"] == before, f"{op}: the refresh allocated"
            ctx.synchronize()
            F = A.apply(op, thunk)
            _assert_same_tiling(R, F, f"refresh {op}", op)
            with pytest.raises(pkg.PemError) as e:              # the plan on R is stale until its step 3
                down.export_csr()
            assert e.value.status == state
            down.step3()
            fresh = pkg.CPlan(ctx, A, F)
            fresh.spgemm()
            assert _same_results(down.export_csr(), fresh.export_csr()), f"refresh {op}: the plan after its step 3"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ("powerlaw_600", "rect_33x65_AAt"))
def test_scale_refresh_equals_fresh(pkg, ctx, name, dtype):
    rows, cols, I, J, V = _case(name, dtype)
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=dtype)
    X = pkg.Tiled.from_coo(ctx, cols, rows, J, I, np.asarray(V), dtype=dtype)
    rng = np.random.default_rng(43)
    r0, c0 = _dev(*_vectors(rows, cols, dtype))
    for op in ("times", "plus", "min", "land"):
        for build_mode in ("both", "rows"):
            R = A.scale(*_pick(build_mode, r0, c0), op)
            down = pkg.CPlan(ctx, X, R)
            down.spgemm()
            for k, mode in enumerate(("both", "cols", "neither", "rows")):   # vectors that differ from the build's, one or both null
                A.set_values(_specials(rng, rng.normal(size=A.nnz)))
                r, c = _dev(*_vectors(rows, cols, dtype, seed=50 + k))
                R.set_values_from_scale(A, *_pick(mode, r, c))
                ctx.synchronize()
                F = A.scale(*_pick(mode, r, c), op)
                _assert_same_tiling(R, F, f"{name} scale refresh {op} {build_mode}->{mode}", op)
                down.step3()
                fresh = pkg.CPlan(ctx, X, F)
                fresh.spgemm()
                assert _same_results(down.export_csr(), fresh.export_csr(), op), f"{name} {op}: vals_t after the refresh"
            # the refreshes above ran between builds and plans that carve buffers of their own: measure two more calls alone
            before = ctx.memory_stats()["block_allocs"]
            R.set_values_from_scale(A, r, c)
            R.set_values_from_scale(A, None, c)
            assert ctx.memory_stats()["block_allocs"] == before, "a later scale refresh allocated"
            ctx.synchronize()


# ---- sources and consumers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_any_tiling_as_source(pkg, ctx, dtype, tmp_path):
    rows, cols, I, J, V, _ = CASES["rect_33x65_AAt"]
    Vd = _specials(np.random.default_rng(8), V).astype(dtype)
    T = pkg.Tiled.from_coo(ctx, rows, cols, I, J, Vd, True, dtype=dtype)        # transpose = 1: its own matrix, cols x rows
    M = pkg.Tiled.from_coo(ctx, rows, cols, I, J, np.asarray(V, dtype), dtype=dtype)
    plan = pkg.CPlan(ctx, M, pkg.Tiled.from_coo(ctx, rows, cols, I, J, np.asarray(V, dtype), True, dtype=dtype))
    plan.spgemm()
    sources = dict(transposed=T, cplan=pkg.Tiled.from_cplan(plan), cplan_t=pkg.Tiled.from_cplan(plan, True), select=T.select("triu", -3),
                   extract=T.extract(np.arange(60, 2, -3), np.arange(1, 30)))
    path = str(tmp_path / "t.pemtile")
    T.save(path)
    sources.update(loaded=pkg.Tiled.load(ctx, path), ewise=pkg.Tiled.ewise(T, sources["select"], "times"), transpose=M.transpose(),
                   assign=T.assign(sources["extract"], np.arange(60, 2, -3), np.arange(1, 30), accum="plus"))
    for label, S in sources.items():
        rp, ci, v = S.export_csr()
        sI = np.repeat(np.arange(S.rows, dtype=np.int32), np.diff(rp))
        r, c = _vectors(S.rows, S.cols, dtype, seed=21)
        for op, th in (("rminus", 1.5), ("sqrt", 0), ("powi", 4)):
            want = pkg.Tiled.from_coo(ctx, S.rows, S.cols, sI, ci, ap.apply(v, op, th, dtype), dtype=dtype)
            _assert_same_tiling(S.apply(op, th), want, f"{label} apply {op}")
        for op in ("times", "max"):
            want = pkg.Tiled.from_coo(ctx, S.rows, S.cols, sI, ci, ap.scale(sI, ci, v, r, c, op, dtype), dtype=dtype)
            _assert_same_tiling(_scaled(pkg, S, r, c, op), want, f"{label} scale {op}", op)


def test_results_feed_other_operations_and_round_trip(pkg, ctx, tmp_path):
    import ewiseref
    import selectref
    rows, cols, I, J, V = _case("powerlaw_600", np.float64)
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    r, c = _vectors(rows, cols, np.float64)
    for label, R, Vr in (("apply", A.apply("rdiv", 2.0), ap.apply(V, "rdiv", 2.0)), ("scale", _scaled(pkg, A, r, c, "times"), ap.scale(I, J, V, r, c))):
        assert R.conv_ms > 0
        path = str(tmp_path / f"{label}.pemtile")
        R.save(path)
        _assert_same_tiling(pkg.Tiled.load(ctx, path), R, f"{label}: save / load")
        s = selectref.select(I, J, Vr, "abs_gt", 0.5, np.float64)
        _assert_same_tiling(R.select("abs_gt", 0.5), pkg.Tiled.from_coo(ctx, rows, cols, *s), f"{label} -> select")
        e = ewiseref.ewise(cols, (I, J, Vr), (I, J, V), "plus")
        _assert_same_tiling(pkg.Tiled.ewise(R, A, "plus"), pkg.Tiled.from_coo(ctx, rows, cols, *e), f"{label} -> ewise")
        sub = np.arange(5, 400, 3)
        keep = np.isin(I, sub) & np.isin(J, sub)
        pos = {int(x): k for k, x in enumerate(sub)}
        eI = np.array([pos[int(i)] for i in I[keep]], np.int32)
        eJ = np.array([pos[int(j)] for j in J[keep]], np.int32)
        _assert_same_tiling(R.extract(sub, sub), pkg.Tiled.from_coo(ctx, len(sub), len(sub), eI, eJ, Vr[keep]), f"{label} -> extract")
        _assert_same_tiling(R.apply("abs").apply("sqrt"), pkg.Tiled.from_coo(ctx, rows, cols, I, J, ap.apply(ap.apply(Vr, "abs"), "sqrt")),
                            f"{label} -> apply -> apply")


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg, ctx):
    L = pkg.lib()
    rows, cols, I, J, V, _ = CASES["rand_300"]
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    A32 = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=np.float32)
    h = C.c_void_p()

    def apply(a, op, thunk, out=True, c=ctx._h):
        h.value = 12345
        s = L.pem_tiled_apply(c, a, op, C.c_double(thunk), C.byref(h) if out else None)
        return s, h.value

    def scale(fn, a, op, out=True, c=ctx._h):
        h.value = 12345
        s = fn(c, a, op, None, None, C.byref(h) if out else None)
        return s, h.value

    for op in (-1, 14, 100):
        assert apply(A._h, op, 0.0) == (PEM_E_INVALID, None), op
    for k in (0.0, 65.0, 2.5, np.inf, -1.0, np.nan):
        assert apply(A._h, 13, k) == (PEM_E_INVALID, None), k
    assert apply(None, 0, 0.0) == (PEM_E_INVALID, None)
    assert apply(A._h, 0, 0.0, c=None) == (PEM_E_INVALID, None)
    assert apply(A._h, 0, 0.0, out=False)[0] == PEM_E_INVALID
    for op in (-1, 6, 14):
        assert scale(L.pem_tiled_scale, A._h, op) == (PEM_E_INVALID, None), op
    assert scale(L.pem_tiled_scale, None, 0) == (PEM_E_INVALID, None)
    assert scale(L.pem_tiled_scale, A._h, 0, c=None) == (PEM_E_INVALID, None)
    assert scale(L.pem_tiled_scale, A._h, 0, out=False)[0] == PEM_E_INVALID
    assert scale(L.pem_tiled_scale_f32, A._h, 1) == (PEM_E_INVALID, None)        # _f32 on an fp64 tiling
    assert scale(L.pem_tiled_scale, A32._h, 1) == (PEM_E_INVALID, None)          # and the reverse
    # a NaN thunk is accepted and propagates
    N = A.apply("plus", np.nan)
    assert N.nnz == A.nnz and np.isnan(N.array("vals")).all()
    # the Python layer: names, vector types and lengths
    with pytest.raises(ValueError):
        A.apply("exp")
    with pytest.raises(ValueError):
        A.scale(op="minus")
    good = torch.ones(rows, dtype=torch.float64, device="cuda")
    for bad in (torch.ones(rows + 1, dtype=torch.float64, device="cuda"), torch.ones(rows, dtype=torch.float32, device="cuda"),
                torch.ones(rows, dtype=torch.float64), np.ones(rows), torch.ones(2 * rows, dtype=torch.float64, device="cuda")[::2]):
        with pytest.raises(ValueError):
            A.scale(rows=bad)
        with pytest.raises(ValueError):
            A.scale(rows=good, cols=bad)
    torch.cuda.synchronize()
    # refreshes: null arguments, another A, a tiling made by another operation, the wrong value type, an A recreated after destroy
    R, S, Q = A.apply("abs"), A.scale(good, None), A.select("tril", 0)
    S32 = A32.scale()
    A2 = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    assert L.pem_tiled_set_values_from_apply(None, R._h, A._h) == PEM_E_INVALID
    assert L.pem_tiled_set_values_from_apply(ctx._h, None, A._h) == PEM_E_INVALID
    assert L.pem_tiled_set_values_from_apply(ctx._h, R._h, None) == PEM_E_INVALID
    assert L.pem_tiled_set_values_from_scale(None, S._h, A._h, None, None) == PEM_E_INVALID
    assert L.pem_tiled_set_values_from_scale(ctx._h, None, A._h, None, None) == PEM_E_INVALID
    assert L.pem_tiled_set_values_from_scale(ctx._h, S._h, None, None, None) == PEM_E_INVALID
    assert L.pem_tiled_set_values_from_scale_f32(ctx._h, S._h, A._h, None, None) == PEM_E_INVALID
    assert L.pem_tiled_set_values_from_scale(ctx._h, S32._h, A32._h, None, None) == PEM_E_INVALID
    for t, fn in ((R, "set_values_from_apply"), (S, "set_values_from_scale")):
        for src in (A2, R, S):
            with pytest.raises(pkg.PemError) as e:
                getattr(t, fn)(src)
            assert e.value.status == PEM_E_INVALID
    for fn in ("set_values_from_apply", "set_values_from_scale"):
        with pytest.raises(pkg.PemError) as e:
            getattr(Q, fn)(A)                                   # made by select
        assert e.value.status == PEM_E_INVALID
    with pytest.raises(pkg.PemError):
        R.set_values_from_scale(A)                              # made by apply
    with pytest.raises(pkg.PemError):
        S.set_values_from_apply(A)                              # made by scale
    R.set_values_from_apply(A)
    S.set_values_from_scale(A, good)
    S32.set_values_from_scale(A32)
    ctx.synchronize()
    A.close()                                                   # a tiling recreated (possibly at the same address)
    A3 = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    with pytest.raises(pkg.PemError):
        R.set_values_from_apply(A3)
    with pytest.raises(pkg.PemError):
        S.set_values_from_scale(A3)


def test_empty_tiling(pkg, ctx):
    E = pkg.Tiled.from_coo(ctx, 40, 33, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    r, c = _dev(np.ones(40), np.ones(33))
    for R in (E.apply("minv"), E.scale(r, c, "plus")):
        _assert_same_tiling(R, E, "empty")
        rp, ci, v = R.export_csr()
        assert np.array_equal(rp, np.zeros(41, np.int32)) and len(ci) == len(v) == 0
    E.apply("abs").set_values_from_apply(E)
    S = E.scale(r, c)
    S.set_values_from_scale(E, r, None)
    p = pkg.CPlan(ctx, S, pkg.Tiled.from_coo(ctx, 33, 5, [0], [0], [1.0]))
    p.spgemm()
    assert p.info()["nnz_c"] == 0


# ---- large dimensions -------------------------------------------------------------------------------------------------------------------
def test_large_dimensions(pkg, ctx):
    """more than 262 144 tile rows; the vectors have 4 194 325 entries"""
    n, I, J, V, _ = hypersparse()
    A = pkg.Tiled.from_coo(ctx, n, n, I, J, V)
    assert A.tile_rows > 262_144
    rp, ci, v = A.export_csr()
    eI = np.repeat(np.arange(n, dtype=np.int32), np.diff(rp))
    rng = np.random.default_rng(99)
    r, c = rng.normal(size=n), rng.normal(size=n)
    R = _scaled(pkg, A, r, c, "times")
    got = R.export_csr()
    assert np.array_equal(got[0], rp) and np.array_equal(got[1], ci)
    assert _same_vals(got[2], ap.scale(eI, ci, v, r, c, "times"))
    N = A.apply("ainv")
    got = N.export_csr()
    assert np.array_equal(got[0], rp) and np.array_equal(got[1], ci)
    assert _same_vals(got[2], ap.apply(v, "ainv"))
    x, = _dev(rng.normal(size=n))
    want = pkg.Tiled.from_coo(ctx, n, n, eI, ci, ap.scale(eI, ci, v, r, c, "times"))
    y, yw = R.mxv(x, transpose=True), want.mxv(x, transpose=True)
    ctx.synchronize()
    assert _same_vals(y.cpu().numpy(), yw.cpu().numpy())
