"""GPU: a tiling times a dense row-major block of vectors (pem_tiled_spmm).

The central check: column c of A.spmm(X) equals, bit for bit, A.mxv(X[:, c]) -- with the same old column under accumulate -- under
every semiring, both orientations and k around every width the library compiles (4, 8, 16); zero signs under min/max are the one
allowed difference, NaN payloads are not compared.  X and Y are column slices of wider row-major buffers, and Y's columns past k are
poisoned beforehand and must come back unchanged.  spmmref (mxvref per column) and the plan route (X as a dense tiling) are checked
on smaller sets.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import mxvref as mr
import spmmref as spr
from matgen import cases

pytestmark = pytest.mark.gpu

torch.cuda.is_available()   # (torch's runtime first, as in the other GPU files)

CASES = cases()
PEM_E_INVALID = -1
DTYPES = (np.float64, np.float32)
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3.0e-310, 1.0e-40, 0.5, -0.5, 2.0])
MINMAX = ("min_plus", "max_plus", "max_times")
KS = (1, 3, 4, 5, 7, 8, 9, 13, 15, 16, 17, 21, 37, 69)   # W - 1, W, W + 1 and 2W + 5 for the widths 4, 8, 16
BIG = ("wide_tilecols", "k64_bins", "hub_tile_2100_AAt", "blockrows_10000")


@pytest.fixture(scope="module")
def tctx(pkg):
    """a context on a torch stream made current for the module (as in test_gpu_mxv.py)"""
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


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int32)


def _same_dev(got, want, kind="plus_times"):
    """bit equality on the device (NaN == NaN; +0 == -0 under min/max)"""
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    ok = (_bits(got) == _bits(want)) | (torch.isnan(got) & torch.isnan(want))
    if kind in MINMAX:
        ok |= (got == 0) & (want == 0)
    return bool(ok.all().item())


def _same(got, want, kind="plus_times"):
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    ok = (got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want))
    if kind in MINMAX:
        ok |= (got == 0) & (want == 0)
    return bool(np.all(ok))


def _specials(shape, seed, dtype, base=None):
    """values with about a quarter replaced by +-0, +-inf, NaN and subnormals"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(shape) if base is None else np.array(base, np.float64)
    sp = rng.random(v.shape) < 0.25
    v[sp] = rng.choice(SPECIAL, int(sp.sum()))
    return v.astype(dtype)


def _coo_csr(rows, I, J, V):
    I, J = np.asarray(I, np.int64), np.asarray(J, np.int64)
    o = np.lexsort((J, I))
    rp = np.zeros(rows + 1, np.int64)
    np.cumsum(np.bincount(I, minlength=rows), out=rp[1:])
    return rp, J[o], np.asarray(V)[o]


def _csr_of(case, dtype):
    rows, cols, I, J, V, _ = case
    W = _specials(len(V), rows * 7 + cols, dtype, V)
    return rows, cols, _coo_csr(rows, I, J, W)


def _tiled(pkg, ctx, rows, cols, csr, dtype, transpose=False):
    rp, ci, v = csr
    I = np.repeat(np.arange(rows, dtype=np.int32), np.diff(rp))
    return pkg.Tiled.from_coo(ctx, rows, cols, I, np.asarray(ci, np.int32), v, transpose, dtype=dtype)


def _mxv_cols(A, X, k, s, tr, Y0=None):
    """the per-column mxv of the first k columns of X (on the device), from the old columns of Y0 under accumulate"""
    ny = A.cols if tr else A.rows
    out = torch.empty((k, ny), dtype=X.dtype, device=X.device)
    for c in range(k):
        if Y0 is not None:
            out[c].copy_(Y0[:, c])
        A.mxv(X[:, c].contiguous(), s, transpose=tr, out=out[c], accumulate=Y0 is not None)
    return out.t()


def _check(A, label, ks=KS, seed=0, ref=None):
    """every semiring x orientation x accumulate x k of ks against per-column mxv, X and Y column slices (ld = k + 3 .. k + 11) and
    Y's padding poisoned; ref = (oracle, rows, cols, csr): also against spmmref for the k of ks[1]"""
    dt = torch.float64 if A.value_bytes == 8 else torch.float32
    npdt = np.float64 if A.value_bytes == 8 else np.float32
    kmax = max(ks)
    for tr in (False, True):
        nx, ny = (A.rows, A.cols) if tr else (A.cols, A.rows)
        Xh = _specials((nx, kmax + 11), seed + 11 + tr, npdt)
        Y0h = _specials((ny, kmax + 3), seed + 13 + tr, npdt)
        X, Y0 = _dev(Xh), _dev(Y0h)
        for s in mr.SEMIRINGS:
            for acc in (False, True):
                want = _mxv_cols(A, X, kmax, s, tr, Y0 if acc else None)
                for k in ks:
                    Yfull = Y0.clone()
                    r = A.spmm(X[:, :k], s, transpose=tr, out=Yfull[:, :k], accumulate=acc)
                    assert r.data_ptr() == Yfull.data_ptr()
                    assert _same_dev(Yfull[:, :k], want[:, :k], s), f"{label} {s} transpose={tr} accumulate={acc} k={k}: mxv per column"
                    assert torch.equal(_bits(Yfull[:, k:]), _bits(Y0[:, k:])), f"{label} {s} transpose={tr} k={k}: padding written"
                    if ref is not None and k == ks[1]:
                        oracle, rows, cols, (rp, ci, v) = ref
                        want_h = spr.spmm_into(rows, cols, rp, ci, v, Xh[:, :k], Y0h, k, s, npdt, accumulate=acc, oracle=oracle, transpose=tr)
                        assert _same(_host(Yfull), want_h, s), f"{label} {s} transpose={tr} accumulate={acc} k={k}: spmmref"


# ---- every case, dtype, orientation, semiring, accumulate, k ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case(pkg, oracle, tctx, name, dtype):
    rows, cols, csr = _csr_of(CASES[name], dtype)
    A = _tiled(pkg, tctx, rows, cols, csr, dtype)
    if name in BIG:
        _check(A, name, ks=(1, 5, 17, 33))
    else:
        _check(A, name, ref=(oracle, rows, cols, csr))


# ---- the plan route ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("tiny_9x9", "rand_50", "rect_70x40_AAt", "empty_rows", "dense_48"))
def test_plan_route_with_a_dense_tiling(pkg, tctx, name):
    """Y equals the plan product A*X (X^T... for A^T: (X^T A)^T) with X as a dense tiling storing every entry, scattered into a dense
    array with the start value where C stores nothing"""
    rows, cols, csr = _csr_of(CASES[name], np.float64)
    A = _tiled(pkg, tctx, rows, cols, csr, np.float64)
    k = 6
    for tr in (False, True):
        nx, ny = (rows, cols) if tr else (cols, rows)
        Xh = _specials((nx, k), 31 + tr, np.float64)
        jj, cc = np.meshgrid(np.arange(nx, dtype=np.int32), np.arange(k, dtype=np.int32), indexing="ij")
        if tr:   # X^T (k x nx) * A, transposed back
            XT = pkg.Tiled.from_coo(tctx, k, nx, cc.ravel(), jj.ravel(), Xh.ravel())
        else:
            XD = pkg.Tiled.from_coo(tctx, nx, k, jj.ravel(), cc.ravel(), Xh.ravel())
        for s in mr.SEMIRINGS:
            p = pkg.CPlan(tctx, XT, A, semiring=s) if tr else pkg.CPlan(tctx, A, XD, semiring=s)
            p.spgemm()
            crp, cci, cv = p.export_csr()
            want = np.full((k, ny) if tr else (ny, k), mr.MXV_START[s])
            want[np.repeat(np.arange(len(crp) - 1), np.diff(crp)), cci] = cv
            if tr:
                want = want.T
            got = _host(A.spmm(_dev(Xh), s, transpose=tr))
            assert _same(got, want, s), f"{name} {s} transpose={tr}"


# ---- walk boundaries --------------------------------------------------------------------------------------------------------------
def _walk_matrices():
    rng = np.random.default_rng(5)
    out = {}
    for n in (64, 65, 4097):   # one row of n entries (one chunk, one past a chunk, many chunks)
        J = np.sort(rng.choice(8192, n, replace=False)).astype(np.int32)
        out[f"row_{n}"] = (40, 8192, np.full(n, 17, np.int32), J, rng.standard_normal(n))
    # a tile row with one heavy row (3000 entries) and 15 light ones (3 entries each)
    I = [np.full(3000, 32, np.int32)]
    J = [np.sort(rng.choice(6000, 3000, replace=False)).astype(np.int32)]
    for r in range(33, 48):
        I.append(np.full(3, r, np.int32))
        J.append(np.sort(rng.choice(6000, 3, replace=False)).astype(np.int32))
    I, J = np.concatenate(I), np.concatenate(J)
    out["heavy_row_in_tile_row"] = (64, 6000, I, J, rng.standard_normal(len(I)))
    # a heavy tile column: every row of 3000 has entries in columns 16..31
    I = np.repeat(np.arange(3000, dtype=np.int32), 4)
    J = (16 + np.concatenate([np.sort(rng.choice(16, 4, replace=False)) for _ in range(3000)])).astype(np.int32)
    out["heavy_tile_col"] = (3000, 48, I, J, rng.standard_normal(len(I)))
    return out


WALK = _walk_matrices()


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", sorted(WALK))
def test_walk_boundaries(pkg, tctx, name, dtype):
    rows, cols, I, J, V = WALK[name]
    V = _specials(len(V), 3, dtype, V)
    A = pkg.Tiled.from_coo(tctx, rows, cols, I, J, V, dtype=dtype)
    _check(A, name, ks=(1, 5, 16, 33))


# ---- every origin -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", ("rand_300", "rect_70x40_AAt", "powerlaw_600"))
def test_every_origin(pkg, oracle, tctx, tmp_path, name, dtype):
    """tilings built with transpose = 1, from_cplan C and C^T, ewise, select and save/load"""
    rows, cols, csr = _csr_of(CASES[name], dtype)
    A = _tiled(pkg, tctx, rows, cols, csr, dtype)
    At = _tiled(pkg, tctx, rows, cols, csr, dtype, transpose=True)
    assert (At.rows, At.cols) == (cols, rows)
    p = pkg.CPlan(tctx, A, At)
    p.spgemm()
    path = str(tmp_path / "a.pemt")
    A.save(path)
    origins = {"transposed": At, "from_cplan": pkg.Tiled.from_cplan(p), "from_cplan^T": pkg.Tiled.from_cplan(p, transpose=True),
               "ewise": pkg.Tiled.ewise(A, A, "max"), "select": A.select("tril", 0), "select_value": A.select("abs_gt", 0.3),
               "loaded": pkg.Tiled.load(tctx, path)}
    for label, R in origins.items():
        rp, ci, v = R.export_csr()
        _check(R, f"{name} {label}", ks=(1, 5, 17, 33), ref=(oracle, R.rows, R.cols, (rp.astype(np.int64), ci.astype(np.int64), v)))


# ---- one contiguous vector ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_one_contiguous_column_is_mxv(pkg, tctx, dtype):
    """k = 1 with unit strides (mxv's own kernel) and k = 1 as a column slice (the spmm kernel) both give mxv's bits"""
    rows, cols, csr = _csr_of(CASES["hub_row_4000"], dtype)
    A = _tiled(pkg, tctx, rows, cols, csr, dtype)
    for tr in (False, True):
        nx, ny = (rows, cols) if tr else (cols, rows)
        Xw = _dev(_specials((nx, 3), 41 + tr, dtype))
        Y0 = _dev(_specials((ny, 1), 43 + tr, dtype))
        for s in mr.SEMIRINGS:
            for acc in (False, True):
                want = _mxv_cols(A, Xw, 1, s, tr, Y0 if acc else None)
                Y = Y0.clone()
                A.spmm(Xw[:, :1].contiguous(), s, transpose=tr, out=Y, accumulate=acc)
                assert _same_dev(Y, want, s), f"{s} transpose={tr} accumulate={acc}: contiguous"
                Y = Y0.clone()
                A.spmm(Xw[:, :1], s, transpose=tr, out=Y, accumulate=acc)
                assert _same_dev(Y, want, s), f"{s} transpose={tr} accumulate={acc}: column slice"


# ---- empty inputs -----------------------------------------------------------------------------------------------------------------
def test_empty_tiling_empty_lines_and_zero_columns(pkg, tctx):
    rows, cols, I, J, V, _ = CASES["empty_matrix"]
    E = pkg.Tiled.from_coo(tctx, rows, cols, I, J, V)
    for s in mr.SEMIRINGS:
        for tr in (False, True):
            n = cols if tr else rows
            got = _host(E.spmm(_dev(np.ones((n, 3))), s, transpose=tr))
            assert _same(got, np.full((n, 3), mr.MXV_START[s])), s
            old = _specials((n, 3), 5, np.float64)
            out = _dev(old)
            E.spmm(_dev(np.ones((n, 3))), s, transpose=tr, out=out, accumulate=True)
            assert _same(_host(out), old), f"{s}: accumulate must leave empty rows untouched"
    rows, cols, csr = _csr_of(CASES["empty_rows"], np.float64)
    A = _tiled(pkg, tctx, rows, cols, csr, np.float64)
    _check(A, "empty_rows", ks=(2, 20))
    # k = 0: nothing is written, out comes back with shape (n, 0)
    for tr in (False, True):
        nx, ny = (rows, cols) if tr else (cols, rows)
        r = A.spmm(_dev(np.ones((nx, 0))), transpose=tr)
        assert tuple(r.shape) == (ny, 0)
        buf = _dev(np.full((ny, 4), 7.0))
        A.spmm(_dev(np.ones((nx, 4)))[:, :0], transpose=tr, out=buf[:, :0])
        assert np.all(_host(buf) == 7.0)


# ---- repeat calls, allocations, fresh values ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("blockrows_10000", "hub_row_4000", "xl_mixed_AAt"))
def test_two_calls_identical_and_repeat_call_allocates_nothing(pkg, tctx, name):
    rows, cols, csr = _csr_of(CASES[name], np.float64)
    A = _tiled(pkg, tctx, rows, cols, csr, np.float64)
    for tr in (False, True):
        for k in (3, 40):
            X = _dev(_specials((rows if tr else cols, k), 3, np.float64))
            for s in ("plus_times", "min_plus"):
                y1 = _host(A.spmm(X, s, transpose=tr))
                out = torch.empty((cols if tr else rows, k), dtype=torch.float64, device="cuda")
                before = tctx.memory_stats()["block_allocs"]
                y2 = _host(A.spmm(X, s, transpose=tr, out=out))
                assert tctx.memory_stats()["block_allocs"] == before, f"{name} {s} transpose={tr}: a repeat call allocated"
                assert np.array_equal(y1.view(np.uint64), y2.view(np.uint64)), f"{name} {s} transpose={tr}: two calls differ"


def test_column_schedule_of_mxv_is_reused(pkg, tctx):
    rows, cols, csr = _csr_of(CASES["powerlaw_600"], np.float64)
    A = _tiled(pkg, tctx, rows, cols, csr, np.float64)
    A.mxv(_dev(np.ones(rows)), transpose=True)
    tctx.synchronize()
    before = tctx.memory_stats()["block_allocs"]
    A.spmm(_dev(np.ones((rows, 9))), transpose=True)
    assert tctx.memory_stats()["block_allocs"] == before


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_set_values_device_then_spmm_without_sync(pkg, oracle, tctx, dtype):
    rows, cols, csr = _csr_of(CASES["powerlaw_600"], dtype)
    rp, ci, v = csr
    A = _tiled(pkg, tctx, rows, cols, csr, dtype)
    Xh, XTh = _specials((cols, 6), 21, dtype), _specials((rows, 6), 22, dtype)
    X, XT = _dev(Xh), _dev(XTh)
    A.spmm(XT, transpose=True)   # (the column schedule exists before the refresh)
    for it in range(3):
        v2 = np.random.default_rng(it).standard_normal(len(v)).astype(dtype)
        A.set_values_device(_dev(v2), "row")
        y, yt = A.spmm(X), A.spmm(XT, transpose=True)
        assert _same(_host(y), spr.spmm(rows, cols, rp, ci, v2, Xh, "plus_times", dtype, oracle=oracle)), it
        assert _same(_host(yt), spr.spmm(rows, cols, rp, ci, v2, XTh, "plus_times", dtype, oracle=oracle, transpose=True)), it


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments(pkg, tctx):
    L = pkg.lib()
    rows, cols, csr = _csr_of(CASES["rect_70x40_AAt"], np.float64)
    A = _tiled(pkg, tctx, rows, cols, csr, np.float64)
    F = _tiled(pkg, tctx, rows, cols, csr, np.float32)
    k = 5
    X, Y = _dev(np.ones((cols, k))), _dev(np.zeros((rows, k)))
    XF, YF = _dev(np.ones((cols, k), np.float32)), _dev(np.zeros((rows, k), np.float32))
    px, py = C.c_void_p(X.data_ptr()), C.c_void_p(Y.data_ptr())
    i64 = C.c_int64

    def sp(ctx=tctx._h, T=A._h, s=0, tr=0, kk=k, x=px, ldx=k, y=py, ldy=k, acc=0, fn=L.pem_tiled_spmm):
        return fn(ctx, T, s, tr, i64(kk), x, i64(ldx), y, i64(ldy), acc)

    assert sp() == 0
    bad = [sp(ctx=None), sp(T=None), sp(s=6), sp(s=-1), sp(tr=2), sp(tr=-1), sp(acc=2), sp(kk=-1), sp(ldx=k - 1), sp(ldy=k - 1),
           sp(kk=0, ldx=0), sp(kk=0, ldy=0), sp(x=None), sp(y=None),
           sp(fn=L.pem_tiled_spmm_f32, x=C.c_void_p(XF.data_ptr()), y=C.c_void_p(YF.data_ptr())),   # fp64 tiling, fp32 entry
           sp(T=F._h),                                                                              # fp32 tiling, fp64 entry
           sp(ldx=2 ** 62), sp(ldy=2 ** 62)]                                                        # n * ld overflows int64
    assert bad == [PEM_E_INVALID] * len(bad)
    # null pointers are fine where the block is empty
    assert sp(kk=0, x=None, y=None, ldx=1, ldy=1) == 0
    # overlapping spans: the same buffer, Y starting inside X, and X's last row reaching into Y
    buf = _dev(np.ones(cols * k + rows * k))
    p0 = buf.data_ptr()
    assert sp(x=C.c_void_p(p0), y=C.c_void_p(p0)) == PEM_E_INVALID
    assert sp(x=C.c_void_p(p0), y=C.c_void_p(p0 + 8 * (cols * k - 1))) == PEM_E_INVALID
    assert sp(x=C.c_void_p(p0), y=C.c_void_p(p0 + 8 * cols * k)) == 0   # adjacent is fine
    # X with ld = k + 2: its span ends at (cols - 1) * (k + 2) + k, so Y may start there but not one element earlier
    end = (cols - 1) * (k + 2) + k
    big = _dev(np.ones(end + rows * k))
    q0 = big.data_ptr()
    assert sp(x=C.c_void_p(q0), ldx=k + 2, y=C.c_void_p(q0 + 8 * end)) == 0
    assert sp(x=C.c_void_p(q0), ldx=k + 2, y=C.c_void_p(q0 + 8 * (end - 1))) == PEM_E_INVALID
    tctx.synchronize()
    # the Python layer: 1-D input, column-major views, the wrong dtype, device or shape, names
    for bad_x in (_dev(np.ones(cols)), X.t().contiguous().t()[:, :], _dev(np.ones((cols, k), np.float32)), np.ones((cols, k)),
                  _dev(np.ones((cols + 1, k))), _dev(np.ones((k, cols))).t(), torch.ones((cols, k), dtype=torch.float64)):
        with pytest.raises(ValueError, match="want a 2-D device tensor"):
            A.spmm(bad_x)
    with pytest.raises(ValueError, match="want a 2-D device tensor"):
        A.spmm(X, out=_dev(np.zeros((rows, k + 1))))
    with pytest.raises(ValueError, match="want a 2-D device tensor"):
        A.spmm(X, out=_dev(np.zeros((rows + 1, k))))
    with pytest.raises(ValueError, match="want a 2-D device tensor"):
        A.spmm(X, transpose=True)
    with pytest.raises(ValueError):
        A.spmm(X, "plus_min")
    if torch.cuda.device_count() > 1:   # a tensor on another device than the context's
        with pytest.raises(ValueError, match="want a 2-D device tensor"):
            A.spmm(X.to("cuda:1"))


# ---- full size ----------------------------------------------------------------------------------------------------------------
def test_full_size_webbase(pkg, standins, tctx):
    """the numpy webbase-1M stand-in at k = 16, rows and columns, against per-column mxv"""
    rows, cols, I, J, V = standins.make("webbase-1M", 1.0)
    A = pkg.Tiled.from_coo(tctx, rows, cols, I, J, V)
    k = 16
    for tr in (False, True):
        X = _dev(np.random.default_rng(7 + tr).standard_normal((A.rows if tr else A.cols, k)))
        for s in ("plus_times", "min_plus"):
            got = A.spmm(X, s, transpose=tr)
            assert _same_dev(got, _mxv_cols(A, X, k, s, tr), s), f"webbase-1M {s} transpose={tr}"
