"""GPU: matrix-vector products and reductions of tilings (pem_tiled_mxv / pem_tiled_reduce).

The central checks: A.mxv(x) equals, bit for bit, the plan product A*X (X: the cols x 1 tiling storing every x_j) scattered into a
dense vector with the start value at empty rows -- and X^T*A for the transposed orientation -- under every semiring; and it equals
mxvref's fold, with and without accumulate.  Zero signs under min/max are the one allowed difference, NaN payloads are not compared.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import mxvref as mr
from matgen import cases

pytestmark = pytest.mark.gpu

torch.cuda.is_available()   # (torch's runtime first, as in the other GPU files)

CASES = cases()
PEM_E_INVALID = -1
DTYPES = (np.float64, np.float32)
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3.0e-310, 1.0e-40, 0.5, -0.5, 2.0])
MINMAX = ("min_plus", "max_plus", "max_times", "min", "max")


@pytest.fixture(scope="module")
def tctx(pkg):
    """a context on a torch stream made current for the module: torch's work and the library's calls are ordered with no extra sync
    (torch's default stream is the null stream, which pem_ctx_create_on_stream does not take: NULL means a stream of its own)"""
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


def _specials(n, seed, dtype, base=None):
    """a vector with about a quarter replaced by +-0, +-inf, NaN and subnormals"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n) if base is None else np.array(base, np.float64)
    sp = rng.random(n) < 0.25
    v[sp] = rng.choice(SPECIAL, int(sp.sum()))
    return v.astype(dtype)


def _csr_of(case, dtype):
    rows, cols, I, J, V, _ = case
    W = _specials(len(V), rows * 7 + cols, dtype, V)
    return rows, cols, _coo_csr(rows, I, J, W)


def _coo_csr(rows, I, J, V):
    I, J = np.asarray(I, np.int64), np.asarray(J, np.int64)
    o = np.lexsort((J, I))
    rp = np.zeros(rows + 1, np.int64)
    np.cumsum(np.bincount(I, minlength=rows), out=rp[1:])
    return rp, J[o], np.asarray(V)[o]


def _tiled(pkg, ctx, rows, cols, csr, dtype, transpose=False):
    rp, ci, v = csr
    I = np.repeat(np.arange(rows, dtype=np.int32), np.diff(rp))
    if transpose:   # the tiling of M^T from M's COO
        return pkg.Tiled.from_coo(ctx, rows, cols, I, np.asarray(ci, np.int32), v, True, dtype=dtype)
    return pkg.Tiled.from_coo(ctx, rows, cols, I, np.asarray(ci, np.int32), v, dtype=dtype)


def _plan_route(pkg, ctx, A, x, semiring, transpose):
    """A*X (X^T*A) scattered into a dense vector, the start value where C stores nothing"""
    dt = A.dtype
    n = len(x)
    if transpose:
        X = pkg.Tiled.from_coo(ctx, 1, n, np.zeros(n, np.int32), np.arange(n, dtype=np.int32), x, dtype=dt)
        p = pkg.CPlan(ctx, X, A, semiring=semiring)
    else:
        X = pkg.Tiled.from_coo(ctx, n, 1, np.arange(n, dtype=np.int32), np.zeros(n, np.int32), x, dtype=dt)
        p = pkg.CPlan(ctx, A, X, semiring=semiring)
    p.spgemm()
    rp, ci, v = p.export_csr()
    ny = A.cols if transpose else A.rows
    y = np.full(ny, mr.MXV_START[semiring], dt)
    if transpose:
        y[ci] = v
    else:
        y[np.diff(rp) > 0] = v
    return y


def _check_all(pkg, oracle, ctx, A, rows, cols, csr, dtype, label, plan_route=True, seed=0):
    """every semiring x orientation x accumulate, and every reduce op x dim x accumulate, against mxvref (and the plan route)"""
    rp, ci, v = csr
    for tr in (False, True):
        nx, ny = (rows, cols) if tr else (cols, rows)
        x = _specials(nx, seed + 11 + tr, dtype)
        y0 = _specials(ny, seed + 13 + tr, dtype)
        dx = _dev(x)
        for s in mr.SEMIRINGS:
            got = _host(A.mxv(dx, s, transpose=tr))
            want = mr.mxv(rows, cols, rp, ci, v, x, s, dtype, oracle=oracle, transpose=tr)
            assert _same(got, want, s), f"{label} {s} transpose={tr}: mxvref"
            if plan_route:
                assert _same(got, _plan_route(pkg, ctx, A, x, s, tr), s), f"{label} {s} transpose={tr}: plan route"
            out = _dev(y0)
            r = A.mxv(dx, s, transpose=tr, out=out, accumulate=True)
            assert r is out
            want = mr.mxv(rows, cols, rp, ci, v, x, s, dtype, y0=y0, oracle=oracle, transpose=tr)
            assert _same(_host(out), want, s), f"{label} {s} transpose={tr} accumulate"
    for dim in ("rows", "cols"):
        n = cols if dim == "cols" else rows
        y0 = _specials(n, seed + 17, dtype)
        for op in mr.OPS:
            got = _host(A.reduce(op, dim))
            assert _same(got, mr.reduce(rows, cols, rp, ci, v, op, dtype, dim=dim), op), f"{label} reduce {op} {dim}"
            out = _dev(y0)
            A.reduce(op, dim, out=out, accumulate=True)
            assert _same(_host(out), mr.reduce(rows, cols, rp, ci, v, op, dtype, y0=y0, dim=dim), op), f"{label} reduce {op} {dim} acc"
        tr = dim == "cols"
        nx = rows if tr else cols
        one, zero = _dev(np.ones(nx, dtype)), _dev(np.zeros(nx, dtype))
        assert _same(_host(A.reduce("plus", dim)), _host(A.mxv(one, "plus_times", transpose=tr))), f"{label} plus == mxv(x = 1)"
        assert _same(_host(A.reduce("min", dim)), _host(A.mxv(zero, "min_plus", transpose=tr)), "min"), f"{label} min"
        assert _same(_host(A.reduce("max", dim)), _host(A.mxv(zero, "max_plus", transpose=tr)), "max"), f"{label} max"
        assert _same(_host(A.reduce("lor", dim)), _host(A.mxv(one, "lor_land", transpose=tr))), f"{label} lor"


# ---- every case, dtype, orientation, semiring, op -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case(pkg, oracle, tctx, name, dtype):
    rows, cols, csr = _csr_of(CASES[name], dtype)
    A = _tiled(pkg, tctx, rows, cols, csr, dtype)
    _check_all(pkg, oracle, tctx, A, rows, cols, csr, dtype, name)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", ("rand_300", "rect_70x40_AAt", "rect_33x65_AAt", "ragged_37", "powerlaw_600", "hub_row_4000", "empty_rows"))
def test_transposed_tiling_acts_as_its_matrix(pkg, oracle, tctx, name, dtype):
    """a tiling built with transpose = 1 represents M^T: its rows are M's columns"""
    rows, cols, csr = _csr_of(CASES[name], dtype)
    T = _tiled(pkg, tctx, rows, cols, csr, dtype, transpose=True)
    assert (T.rows, T.cols) == (cols, rows)
    tcsr = mr.transpose_csr(rows, cols, *csr)
    _check_all(pkg, oracle, tctx, T, cols, rows, tcsr, dtype, f"{name}^T")


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", ("rand_300", "powerlaw_600", "band_1500", "rect_70x40_AAt"))
def test_derived_tilings(pkg, oracle, tctx, name, dtype):
    """operands made by from_cplan (C and C^T), ewise and select: checked against mxvref on their own export"""
    rows, cols, csr = _csr_of(CASES[name], dtype)
    A = _tiled(pkg, tctx, rows, cols, csr, dtype)
    At = _tiled(pkg, tctx, rows, cols, csr, dtype, transpose=True)
    p = pkg.CPlan(tctx, A, At)
    p.spgemm()
    derived = {"from_cplan": pkg.Tiled.from_cplan(p), "from_cplan^T": pkg.Tiled.from_cplan(p, transpose=True),
               "ewise": pkg.Tiled.ewise(A, A, "max"), "select": A.select("tril", 0), "select_value": A.select("abs_gt", 0.3)}
    for label, R in derived.items():
        rp, ci, v = R.export_csr()
        _check_all(pkg, oracle, tctx, R, R.rows, R.cols, (rp.astype(np.int64), ci.astype(np.int64), v), dtype, f"{name} {label}",
                   plan_route=label in ("from_cplan", "select"))


# ---- stream order, determinism, allocations -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("blockrows_10000", "hub_row_4000", "xl_mixed_AAt"))
def test_two_calls_identical_and_second_call_allocates_nothing(pkg, tctx, name):
    rows, cols, csr = _csr_of(CASES[name], np.float64)
    A = _tiled(pkg, tctx, rows, cols, csr, np.float64)
    for tr in (False, True):
        x = _dev(_specials(rows if tr else cols, 3, np.float64))
        for s in ("plus_times", "min_plus"):
            y1 = _host(A.mxv(x, s, transpose=tr))
            out = torch.empty(cols if tr else rows, dtype=torch.float64, device="cuda")
            before = tctx.memory_stats()["block_allocs"]
            y2 = _host(A.mxv(x, s, transpose=tr, out=out))
            A.reduce("plus", "cols" if tr else "rows", out=out)
            assert tctx.memory_stats()["block_allocs"] == before, f"{name} {s} transpose={tr}: a repeat call allocated"
            assert np.array_equal(y1.view(np.uint64), y2.view(np.uint64)), f"{name} {s} transpose={tr}: two calls differ"


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_set_values_device_then_mxv_without_sync(pkg, oracle, tctx, dtype):
    rows, cols, csr = _csr_of(CASES["powerlaw_600"], dtype)
    rp, ci, v = csr
    A = _tiled(pkg, tctx, rows, cols, csr, dtype)
    x, xt = _specials(cols, 21, dtype), _specials(rows, 22, dtype)
    dx, dxt = _dev(x), _dev(xt)
    A.mxv(dxt, transpose=True)   # (the column schedule exists before the refresh)
    for k in range(3):
        v2 = np.random.default_rng(k).standard_normal(len(v)).astype(dtype)
        A.set_values_device(_dev(v2), "row")
        y, yt = A.mxv(dx), A.mxv(dxt, transpose=True)
        assert _same(_host(y), mr.mxv(rows, cols, rp, ci, v2, x, "plus_times", dtype, oracle=oracle)), k
        assert _same(_host(yt), mr.mxv(rows, cols, rp, ci, v2, xt, "plus_times", dtype, oracle=oracle, transpose=True)), k


def test_power_iteration_on_the_device_equals_the_host_chain(pkg, oracle, tctx):
    rows, cols, I, J, V, _ = CASES["rand_300"]
    rp, ci, v = _coo_csr(rows, I, J, np.asarray(V, np.float64) * 0.25)
    A = _tiled(pkg, tctx, rows, cols, (rp, ci, v), np.float64)
    x0 = np.random.default_rng(4).standard_normal(cols)
    x = _dev(x0)
    y = torch.empty_like(x)
    for _ in range(20):   # x <- (A x) / 2 + x0 / 4, all on the device
        A.mxv(x, out=y)
        x = y * 0.5 + _dev(x0) * 0.25
    h = x0.copy()
    for _ in range(20):
        h = mr.mxv(rows, cols, rp, ci, v, h, "plus_times", np.float64, oracle=oracle) * 0.5 + x0 * 0.25
    assert _same(_host(x), h)


def test_empty_tiling_and_empty_lines(pkg, tctx):
    rows, cols, I, J, V, _ = CASES["empty_matrix"]
    E = pkg.Tiled.from_coo(tctx, rows, cols, I, J, V)
    for s in mr.SEMIRINGS:
        for tr in (False, True):
            y = _host(E.mxv(_dev(np.ones(cols)), s, transpose=tr))
            assert _same(y, np.full(rows, mr.MXV_START[s])), s
            old = _specials(rows, 5, np.float64)
            out = _dev(old)
            E.mxv(_dev(np.ones(cols)), s, transpose=tr, out=out, accumulate=True)
            assert _same(_host(out), old), f"{s}: accumulate must leave empty rows untouched"
    for op in mr.OPS:
        assert _same(_host(E.reduce(op, "cols")), np.full(cols, mr.IDENTITY[op])), op


# ---- errors -----------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments(pkg, tctx):
    L = pkg.lib()
    rows, cols, csr = _csr_of(CASES["rect_70x40_AAt"], np.float64)
    A = _tiled(pkg, tctx, rows, cols, csr, np.float64)
    F = _tiled(pkg, tctx, rows, cols, csr, np.float32)
    x, y = _dev(np.ones(cols)), _dev(np.zeros(rows))
    xf, yf = _dev(np.ones(cols, np.float32)), _dev(np.zeros(rows, np.float32))
    px, py = C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr())
    mxv, red = L.pem_tiled_mxv, L.pem_tiled_reduce
    ok = mxv(tctx._h, A._h, 0, 0, px, py, 0)
    assert ok == 0
    bad = [
        mxv(None, A._h, 0, 0, px, py, 0), mxv(tctx._h, None, 0, 0, px, py, 0), mxv(tctx._h, A._h, 0, 0, None, py, 0),
        mxv(tctx._h, A._h, 0, 0, px, None, 0), mxv(tctx._h, A._h, 6, 0, px, py, 0), mxv(tctx._h, A._h, -1, 0, px, py, 0),
        mxv(tctx._h, A._h, 0, 2, px, py, 0), mxv(tctx._h, A._h, 0, 0, px, py, 2), mxv(tctx._h, A._h, 0, -1, px, py, 0),
        L.pem_tiled_mxv_f32(tctx._h, A._h, 0, 0, C.c_void_p(xf.data_ptr()), C.c_void_p(yf.data_ptr()), 0),   # fp64 tiling, fp32 entry
        mxv(tctx._h, F._h, 0, 0, px, py, 0),                                                                  # fp32 tiling, fp64 entry
        red(None, A._h, 0, 0, py, 0), red(tctx._h, None, 0, 0, py, 0), red(tctx._h, A._h, 0, 0, None, 0), red(tctx._h, A._h, 6, 0, py, 0),
        red(tctx._h, A._h, -1, 0, py, 0), red(tctx._h, A._h, 0, 2, py, 0), red(tctx._h, A._h, 0, 0, py, 2),
        L.pem_tiled_reduce_f32(tctx._h, A._h, 0, 0, C.c_void_p(yf.data_ptr()), 0), red(tctx._h, F._h, 0, 0, py, 0),
    ]
    assert bad == [PEM_E_INVALID] * len(bad)
    # overlapping x and y: the same buffer, and y starting inside x
    buf = _dev(np.ones(cols + rows))
    p0 = buf.data_ptr()
    assert mxv(tctx._h, A._h, 0, 0, C.c_void_p(p0), C.c_void_p(p0), 0) == PEM_E_INVALID
    assert mxv(tctx._h, A._h, 0, 0, C.c_void_p(p0), C.c_void_p(p0 + 8 * (cols - 1)), 0) == PEM_E_INVALID
    assert mxv(tctx._h, A._h, 0, 0, C.c_void_p(p0), C.c_void_p(p0 + 8 * cols), 0) == 0   # adjacent is fine
    assert mxv(tctx._h, A._h, 0, 1, C.c_void_p(p0 + 8 * cols - 8), C.c_void_p(p0), 0) == PEM_E_INVALID   # transposed lengths
    tctx.synchronize()
    # the Python layer: wrong dtype, length, device, contiguity, names
    for bad_x in (np.ones(cols), _dev(np.ones(cols, np.float32)), _dev(np.ones(cols + 1)), _dev(np.ones(2 * cols))[::2]):
        with pytest.raises(ValueError, match="want a contiguous device tensor"):
            A.mxv(bad_x)
    with pytest.raises(ValueError, match="want a contiguous device tensor"):
        A.mxv(x, out=_dev(np.zeros(rows + 1)))
    with pytest.raises(ValueError, match="want a contiguous device tensor"):
        A.reduce("plus", "cols", out=y)
    with pytest.raises(ValueError):
        A.mxv(x, "plus_min")
    with pytest.raises(ValueError):
        A.reduce("minus")
    with pytest.raises(ValueError):
        A.reduce("plus", "diag")


# ---- full size ----------------------------------------------------------------------------------------------------------------
def test_full_size_webbase(pkg, standins, tctx):
    """the numpy webbase-1M stand-in A and its A^2 (from_cplan): mxv against the plan route, reduce against mxvref, rows and columns"""
    rows, cols, I, J, V = standins.make("webbase-1M-r2", 1.0)
    A = pkg.Tiled.from_coo(tctx, rows, cols, I, J, V)
    p = pkg.CPlan(tctx, A, A)
    p.spgemm()
    A2 = pkg.Tiled.from_cplan(p)
    del p
    for label, M in (("A", A), ("A^2", A2)):
        rp, ci, v = M.export_csr()
        for tr in (False, True):
            x0 = np.random.default_rng(7 + tr).standard_normal(M.rows if tr else M.cols)
            x = _dev(x0)
            for s in ("plus_times", "min_plus"):
                got = _host(M.mxv(x, s, transpose=tr))
                assert _same(got, _plan_route(pkg, tctx, M, x0, s, tr), s), f"{label} {s} transpose={tr}"
            for op in ("plus", "max"):
                dim = "cols" if tr else "rows"
                want = mr.reduce(M.rows, M.cols, rp, ci, v, op, np.float64, dim=dim)
                assert _same(_host(M.reduce(op, dim)), want, op), f"{label} reduce {op} {dim}"
