"""GPU: frontier products and breadth-first search of tilings (pem_tiled_mxv_frontier / pem_tiled_bfs).

The central check: A.mxv_frontier equals frontierref's model bit for bit (the `_same` rule of test_gpu_mxv.py) -- the fold over the
entries whose x is present at the allowed outputs, the old y everywhere else -- while the absent x positions hold NaN and +-inf and
A holds the specials of section 3k: a skip that is only an optimisation (the dead entries still multiplied, by a zero say) fails.
The line flags of the mark step equal the model's exactly, so over-marking fails too.

Coverage.  Every case runs both orientations in fp64 and fp32 over twenty (presence, mask, complement) combinations: every presence
pattern without a mask, every mask with and without complement under a random half of x, and four sparse-with-sparse pairs.  Cases
of up to 3000 entries run all six semirings on every combination; the larger ones (whose host model costs tens of milliseconds a
call) two per combination in rotation, which still gives every semiring to at least six combinations.  accumulate alternates over
(combination, semiring), so every semiring sees both values in every case.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import frontierref as fr
import mxvref as mr
from matgen import cases

pytestmark = pytest.mark.gpu

torch.cuda.is_available()   # (torch's runtime first, as in the other GPU files)

CASES = cases()
PEM_E_INVALID, PEM_E_STATE = -1, -6
DTYPES = (np.float64, np.float32)
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3.0e-310, 1.0e-40, 0.5, -0.5, 2.0])
MINMAX = ("min_plus", "max_plus", "max_times")
POISON = np.array([np.nan, np.inf, -np.inf])

# (case, the tiling built with transpose = 1)
TILINGS = [(n, False) for n in ("one_entry", "ragged_37", "dense_tile", "rect_33x65_AAt", "rect_70x40_AAt", "empty_rows", "empty_matrix",
                                "powerlaw_600", "hub_row_4000")] + [("rect_33x65_AAt", True), ("rect_70x40_AAt", True)]
PRESENCE = ("none", "all", "one", "last", "per_segment", "segment", "half", "fiftieth")
MASKS = ("on", "off", "one_per_line", "half")
COMBOS = ([(p, None, False) for p in PRESENCE] + [("half", m, c) for m in MASKS for c in (False, True)]
          + [("fiftieth", "half", True), ("segment", "one_per_line", False), ("per_segment", "half", False), ("one", "one_per_line", True)])


@pytest.fixture(scope="module")
def tctx(pkg):
    """a context on a torch stream made current for the module (see test_gpu_mxv.py)"""
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


def _bits(a):
    return np.asarray(a).view(np.uint64 if np.asarray(a).dtype == np.float64 else np.uint32)


def _specials(n, seed, dtype, base=None):
    """a vector with about a quarter replaced by +-0, +-inf, NaN and subnormals"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n) if base is None else np.array(base, np.float64)
    sp = rng.random(n) < 0.25
    v[sp] = rng.choice(SPECIAL, int(sp.sum()))
    return v.astype(dtype)


def _coo_csr(rows, I, J, V):
    I, J = np.asarray(I, np.int64), np.asarray(J, np.int64)
    o = np.lexsort((J, I))
    rp = np.zeros(rows + 1, np.int64)
    np.cumsum(np.bincount(I, minlength=rows), out=rp[1:])
    return rp, J[o], np.asarray(V)[o]


def _operand(pkg, ctx, name, dtype, transposed=False, specials=True):
    """(tiling, rows, cols, csr) of the matrix the tiling represents"""
    rows, cols, I, J, V, _ = CASES[name]
    W = _specials(len(V), rows * 7 + cols, dtype, V) if specials else np.asarray(V, dtype)
    rp, ci, v = _coo_csr(rows, I, J, W)
    Is = np.repeat(np.arange(rows, dtype=np.int32), np.diff(rp))
    A = pkg.Tiled.from_coo(ctx, rows, cols, Is, np.asarray(ci, np.int32), v, bool(transposed), dtype=dtype)
    if transposed:
        return A, cols, rows, mr.transpose_csr(rows, cols, rp, ci, v)
    return A, rows, cols, (rp, ci, v)


def _presence(kind, n, rng):
    p = np.zeros(n, bool)
    nseg = (n + 15) // 16
    if kind == "all":
        p[:] = True
    elif kind == "one":
        p[n // 3] = True
    elif kind == "last":
        p[n - 1] = True
    elif kind == "per_segment":
        s = np.arange(nseg)
        p[np.minimum(16 * s + (5 * s) % 16, n - 1)] = True
    elif kind == "segment":
        p[16 * (nseg // 2):16 * (nseg // 2) + 16] = True
    elif kind == "half":
        p = rng.random(n) < 0.5
    elif kind == "fiftieth":
        p = rng.random(n) < 0.02
    return p


def _mask(kind, n, rng):
    if kind is None:
        return None
    m = np.zeros(n, bool)
    if kind == "on":
        m[:] = True
    elif kind == "one_per_line":
        L = np.arange((n + 15) // 16)
        m[np.minimum(16 * L + (7 * L) % 16, n - 1)] = True
    elif kind == "half":
        m = rng.random(n) < 0.5
    return m


def _poisoned(x, present):
    """x with NaN, +inf, -inf at the absent positions"""
    x = x.copy()
    absent = np.flatnonzero(~present)
    x[absent] = POISON[np.arange(len(absent)) % 3]
    return x


def _bytes_dev(b, k):
    """the byte array as torch.bool or, every other time, as torch.uint8 holding 0 / 255 (any nonzero byte is on)"""
    return _dev(b) if k % 2 == 0 else _dev(b.astype(np.uint8) * 255)


# ---- every case, dtype, orientation, semiring, presence, mask --------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name,transposed", TILINGS, ids=[n + ("^T" if t else "") for n, t in TILINGS])
def test_every_case_against_the_model(pkg, oracle, tctx, name, transposed, dtype):
    A, rows, cols, (rp, ci, v) = _operand(pkg, tctx, name, dtype, transposed)
    per_combo = 6 if len(ci) <= 3000 else 2
    rng = np.random.default_rng(rows + 3 * cols)
    for tr in (False, True):
        nx, ny = (rows, cols) if tr else (cols, rows)
        x0, y_old = _specials(nx, 11 + tr, dtype), _specials(ny, 13 + tr, dtype)
        # all present, no mask: the dense product, bit for bit, through both forms of "all"
        dx0, ones = _dev(x0), _dev(np.ones(nx, bool))
        for k, s in enumerate(mr.SEMIRINGS):
            acc = bool(k % 2)
            want = _host(A.mxv(dx0, s, transpose=tr, out=_dev(y_old), accumulate=acc))
            got = _host(A.mxv_frontier(dx0, semiring=s, transpose=tr, out=_dev(y_old), accumulate=acc))
            assert _same(got, want, s), f"{name} {s} transpose={tr}: x_present=None differs from mxv"
            got = _host(A.mxv_frontier(dx0, ones, semiring=s, transpose=tr, out=_dev(y_old), accumulate=acc))
            assert _same(got, want, s), f"{name} {s} transpose={tr}: all present differs from mxv"
        for c, (pk, mk, comp) in enumerate(COMBOS):
            present, mask = _presence(pk, nx, rng), _mask(mk, ny, rng)
            x = _poisoned(x0, present)
            dx, dp, dm = _dev(x), _bytes_dev(present, c), None if mask is None else _bytes_dev(mask, c + 1)
            allowed = fr.allowed_of(ny, mask, comp)
            want_flags = fr.line_flags(rows, cols, rp, ci, present, tr)
            for q in range(per_combo):
                s = mr.SEMIRINGS[(per_combo * c + q) % 6]
                acc = bool((c + q) % 2)
                label = f"{name} {s} transpose={tr} present={pk} mask={mk} complement={comp} accumulate={acc}"
                out, opres = _dev(y_old), torch.full((ny,), 7, dtype=torch.uint8, device="cuda")
                r = A.mxv_frontier(None if s == "plus_pair" else dx, dp, dm, comp, s, tr, out, acc, opres)
                assert r is out
                got, gpres = _host(out), _host(opres)
                want, wpres = fr.mxv_frontier(rows, cols, rp, ci, v, x, s, dtype, present, mask, comp, y_old, acc, oracle, tr)
                assert _same(got, want, s), label
                assert np.array_equal(gpres, wpres), f"{label}: out_present"
                assert np.array_equal(_bits(got)[~allowed], _bits(y_old)[~allowed]), f"{label}: a disallowed output was written"
                if acc:
                    quiet = allowed & (wpres == 0)
                    assert np.array_equal(_bits(got)[quiet], _bits(y_old)[quiet]), f"{label}: accumulate touched an output without a term"
                if q == 0:
                    assert np.array_equal(A.frontier_line_flags(tr), want_flags), f"{label}: line flags"


def test_the_poison_bites_the_dense_route(pkg, oracle, tctx):
    """the same x through dense mxv is different: the absent positions of these tests do hold values that would show"""
    differ = 0
    for name in ("ragged_37", "powerlaw_600", "hub_row_4000"):
        A, rows, cols, (rp, ci, v) = _operand(pkg, tctx, name, np.float64, specials=False)
        present = _presence("half", cols, np.random.default_rng(3))
        x = _poisoned(np.random.default_rng(4).standard_normal(cols), present)
        for s in ("plus_times", "min_plus", "max_times", "lor_land"):
            got = _host(A.mxv_frontier(_dev(x), _dev(present), semiring=s))
            want, _ = fr.mxv_frontier(rows, cols, rp, ci, v, x, s, np.float64, present, oracle=oracle)
            assert _same(got, want, s) and not np.isnan(got).any(), f"{name} {s}"
            differ += not _same(got, _host(A.mxv(_dev(x), s)), s)
    assert differ > 0, "dense mxv of the poisoned x equals the frontier result everywhere: the poison shows nothing"


# ---- the plan route ------------------------------------------------------------------------------------------------------------------
def _plan_route(pkg, ctx, A, x, present, semiring, transpose):
    """A*X (X^T*A), X storing exactly the present x_j, scattered into a dense vector with the start value where C stores nothing"""
    dt = A.dtype
    idx = np.flatnonzero(present).astype(np.int32)
    z = np.zeros(len(idx), np.int32)
    n = len(x)
    if transpose:
        X = pkg.Tiled.from_coo(ctx, 1, n, z, idx, x[idx], dtype=dt)
        p = pkg.CPlan(ctx, X, A, semiring=semiring)
    else:
        X = pkg.Tiled.from_coo(ctx, n, 1, idx, z, x[idx], dtype=dt)
        p = pkg.CPlan(ctx, A, X, semiring=semiring)
    p.spgemm()
    rp, ci, v = p.export_csr()
    y = np.full(A.cols if transpose else A.rows, mr.MXV_START[semiring], dt)
    if transpose:
        y[ci] = v
    else:
        y[np.diff(rp) > 0] = v
    return y


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", ("rand_300", "powerlaw_600"))
def test_against_the_plan_product_with_a_sparse_x(pkg, tctx, name, dtype):
    A, rows, cols, _ = _operand(pkg, tctx, name, dtype)
    rng = np.random.default_rng(8)
    for tr in (False, True):
        nx = rows if tr else cols
        for pk in ("half", "fiftieth", "segment"):
            present = _presence(pk, nx, rng)
            x = _poisoned(_specials(nx, 5, dtype), present)
            for s in mr.SEMIRINGS:
                got = _host(A.mxv_frontier(_dev(x), _dev(present), semiring=s, transpose=tr))
                assert _same(got, _plan_route(pkg, tctx, A, x, present, s, tr), s), f"{name} {s} transpose={tr} present={pk}"


# ---- stream order, determinism, allocations ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("powerlaw_600", "hub_row_4000"))
def test_two_calls_identical_and_second_call_allocates_nothing(pkg, tctx, name):
    A, rows, cols, _ = _operand(pkg, tctx, name, np.float64)
    rng = np.random.default_rng(2)
    for tr in (False, True):
        nx, ny = (rows, cols) if tr else (cols, rows)
        present, mask = _dev(_presence("half", nx, rng)), _dev(_mask("half", ny, rng))
        fewer = _dev(_presence("fiftieth", nx, rng))
        x = _dev(_specials(nx, 3, np.float64))
        for s in ("plus_times", "min_plus"):
            y1 = _host(A.mxv_frontier(x, present, mask, True, s, tr, out=torch.zeros(ny, dtype=torch.float64, device="cuda")))
            out, op = torch.zeros(ny, dtype=torch.float64, device="cuda"), torch.zeros(ny, dtype=torch.uint8, device="cuda")
            before = tctx.memory_stats()["block_allocs"]
            y2 = _host(A.mxv_frontier(x, present, mask, True, s, tr, out=out))
            A.mxv_frontier(x, fewer, None, False, s, tr, out=out, out_present=op)
            A.mxv_frontier(x, semiring=s, transpose=tr, out=out)
            assert tctx.memory_stats()["block_allocs"] == before, f"{name} {s} transpose={tr}: a repeat call allocated"
            assert np.array_equal(_bits(y1), _bits(y2)), f"{name} {s} transpose={tr}: two calls differ"


def test_line_flags_hook_states(pkg, tctx):
    A, rows, cols, (rp, ci, v) = _operand(pkg, tctx, "rand_300", np.float64)
    fresh = pkg.Context(0)
    flags = np.zeros(A.tile_rows, np.uint8)
    call = lambda c, n: pkg.lib().pem_test_frontier_line_flags(c._h, flags.ctypes.data_as(C.c_void_p), C.c_int64(n))
    assert call(fresh, A.tile_rows) == PEM_E_STATE   # no frontier call yet
    fresh.close()
    present = _presence("one", cols, None)
    A.mxv_frontier(_dev(np.ones(cols)), _dev(present))
    assert call(tctx, A.tile_rows) == 0
    assert np.array_equal(flags, fr.line_flags(rows, cols, rp, ci, present)) and flags.any()
    assert call(tctx, A.tile_rows + 1) == PEM_E_INVALID
    A.mxv_frontier(_dev(np.ones(cols)))
    assert call(tctx, A.tile_rows) == PEM_E_STATE    # the last call had no x_present: nothing was marked
    tctx.synchronize()


def test_empty_tiling_and_zero_length(pkg, tctx):
    rows, cols, I, J, V, _ = CASES["empty_matrix"]
    E = pkg.Tiled.from_coo(tctx, rows, cols, I, J, V)
    old = _specials(rows, 5, np.float64)
    for s in mr.SEMIRINGS:
        for tr in (False, True):
            pres = torch.full((rows,), 9, dtype=torch.uint8, device="cuda")
            y = _host(E.mxv_frontier(_dev(np.ones(cols)), _dev(np.ones(cols, bool)), semiring=s, transpose=tr, out_present=pres))
            assert _same(y, np.full(rows, mr.MXV_START[s])) and not _host(pres).any(), s
            out = _dev(old)
            E.mxv_frontier(_dev(np.ones(cols)), _dev(np.ones(cols, bool)), semiring=s, transpose=tr, out=out, accumulate=True)
            assert np.array_equal(_bits(_host(out)), _bits(old)), s


# ---- errors ------------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments(pkg, tctx):
    L = pkg.lib()
    A, rows, cols, _ = _operand(pkg, tctx, "rect_70x40_AAt", np.float64)
    F, _, _, _ = _operand(pkg, tctx, "rect_70x40_AAt", np.float32)
    x, y = _dev(np.ones(cols)), _dev(np.zeros(rows))
    xf, yf = _dev(np.ones(cols, np.float32)), _dev(np.zeros(rows, np.float32))
    xp, m, yp = _dev(np.ones(cols, bool)), _dev(np.ones(rows, bool)), _dev(np.zeros(rows, np.uint8))
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    fx, f32 = L.pem_tiled_mxv_frontier, L.pem_tiled_mxv_frontier_f32

    def call(ctx=tctx._h, a=A._h, s=0, tr=0, dx=P(x), dxp=P(xp), dy=P(y), dm=P(m), comp=0, dyp=P(yp), acc=0, fn=fx):
        return fn(ctx, a, s, tr, dx, dxp, dy, dm, comp, dyp, acc)

    assert call() == 0
    assert call(s=4, dx=None) == 0                 # plus_pair reads no x
    assert call(dxp=None, dm=None, dyp=None) == 0
    bad = [call(ctx=None), call(a=None), call(dx=None), call(dy=None), call(s=6), call(s=-1), call(tr=2), call(tr=-1), call(acc=2),
           call(comp=2), call(comp=-1),
           call(fn=f32, dx=P(xf), dy=P(yf)),       # fp64 tiling, fp32 entry
           call(a=F._h)]                           # fp32 tiling, fp64 entry
    assert bad == [PEM_E_INVALID] * len(bad)
    # overlaps: out_present with the mask, x_present, x and y; x with y
    both = _dev(np.ones(2 * rows + cols, np.uint8))
    b0 = both.data_ptr()
    assert call(dm=C.c_void_p(b0), dyp=C.c_void_p(b0 + rows - 1)) == PEM_E_INVALID
    assert call(dm=C.c_void_p(b0), dyp=C.c_void_p(b0 + rows)) == 0               # adjacent is fine
    assert call(dxp=C.c_void_p(b0), dyp=C.c_void_p(b0 + cols - 1)) == PEM_E_INVALID
    assert call(dyp=C.c_void_p(x.data_ptr() + 8 * cols - 1)) == PEM_E_INVALID
    assert call(dyp=C.c_void_p(y.data_ptr())) == PEM_E_INVALID
    buf = _dev(np.ones(cols + rows))
    p0 = buf.data_ptr()
    assert call(dx=C.c_void_p(p0), dy=C.c_void_p(p0 + 8 * (cols - 1))) == PEM_E_INVALID
    assert call(dx=C.c_void_p(p0), dy=C.c_void_p(p0 + 8 * cols)) == 0
    tctx.synchronize()
    # the Python layer: a non-byte tensor, wrong lengths, host arrays, strides, names
    for kw in (dict(x_present=_dev(np.ones(cols, np.int32))), dict(x_present=_dev(np.ones(cols + 1, bool))), dict(x_present=np.ones(cols, bool)),
               dict(mask=_dev(np.ones(rows, np.float64))), dict(mask=_dev(np.ones(cols, bool))), dict(out_present=_dev(np.zeros(rows - 1, np.uint8))),
               dict(out_present=_dev(np.zeros(2 * rows, np.uint8))[::2]), dict(x_present=_dev(np.ones(rows, bool)), transpose=False)):
        with pytest.raises(ValueError, match="want a contiguous device tensor"):
            A.mxv_frontier(x, **kw)
    with pytest.raises(ValueError, match="want a contiguous device tensor"):
        A.mxv_frontier(None)                       # only plus_pair does without x
    with pytest.raises(ValueError, match="want a contiguous device tensor"):
        A.mxv_frontier(xf)
    with pytest.raises(ValueError):
        A.mxv_frontier(x, semiring="plus_min")
    # bfs: not square, source out of range
    lv = torch.empty(rows, dtype=torch.int32, device="cuda")
    d, r = C.c_int32(), C.c_int64()
    assert L.pem_tiled_bfs(tctx._h, A._h, C.c_int64(0), 0, P(lv), C.byref(d), C.byref(r)) == PEM_E_INVALID
    S, n, _, _ = _operand(pkg, tctx, "rand_300", np.float64)
    lv = torch.empty(n, dtype=torch.int32, device="cuda")
    bfs = lambda *a: L.pem_tiled_bfs(*a)
    assert bfs(tctx._h, S._h, C.c_int64(0), 0, P(lv), C.byref(d), C.byref(r)) == 0
    bad = [bfs(tctx._h, S._h, C.c_int64(-1), 0, P(lv), C.byref(d), C.byref(r)), bfs(tctx._h, S._h, C.c_int64(n), 0, P(lv), C.byref(d), C.byref(r)),
           bfs(tctx._h, S._h, C.c_int64(0), 2, P(lv), C.byref(d), C.byref(r)), bfs(None, S._h, C.c_int64(0), 0, P(lv), C.byref(d), C.byref(r)),
           bfs(tctx._h, None, C.c_int64(0), 0, P(lv), C.byref(d), C.byref(r)), bfs(tctx._h, S._h, C.c_int64(0), 0, None, C.byref(d), C.byref(r)),
           bfs(tctx._h, S._h, C.c_int64(0), 0, P(lv), None, C.byref(r)), bfs(tctx._h, S._h, C.c_int64(0), 0, P(lv), C.byref(d), None)]
    assert bad == [PEM_E_INVALID] * len(bad)
    with pytest.raises(pkg.PemError):
        S.bfs(n)


# ---- breadth-first search ------------------------------------------------------------------------------------------------------------
def _bfs_check(T, n, rp, ci, source, label):
    for tr in (False, True):
        lv, depth, reached = T.bfs(source, transpose=tr)
        want, wdepth, wreached = fr.bfs(n, rp, ci, source, tr)
        assert lv.dtype == torch.int32 and np.array_equal(_host(lv), want), f"{label} transpose={tr}: levels"
        assert (depth, reached) == (wdepth, wreached), f"{label} transpose={tr}"
    return wdepth


@pytest.mark.parametrize("name", ("rand_300", "powerlaw_600", "band_1500", "diag_100", "empty_rows"))
def test_bfs_against_the_model(pkg, tctx, name):
    A, n, _, (rp, ci, v) = _operand(pkg, tctx, name, np.float64)   # (the specials include explicit zeros: they are edges)
    deg = np.diff(rp)
    if name == "empty_rows":
        sources = [int(np.flatnonzero(deg == 0)[0]), 0]   # the first has no out-edges
    elif name == "diag_100":
        sources = [41]
    else:
        sources = [0, int(np.argmax(deg)), n - 1]
    for src in sources:
        _bfs_check(A, n, rp, ci, src, f"{name} from {src}")
    if name == "band_1500":
        assert fr.bfs(n, rp, ci, 0)[1] >= 10          # deep: many levels with small frontiers
    if name == "diag_100":
        assert fr.bfs(n, rp, ci, 41)[1:] == (0, 1)    # only the source


def test_bfs_on_an_fp32_tiling_and_on_a_plan_result(pkg, tctx):
    F, n, _, (rp, ci, v) = _operand(pkg, tctx, "powerlaw_600", np.float32)
    _bfs_check(F, n, rp, ci, 7, "fp32")
    A, n, _, _ = _operand(pkg, tctx, "rand_300", np.float64, specials=False)
    p = pkg.CPlan(tctx, A, A)
    p.spgemm()
    A2 = pkg.Tiled.from_cplan(p)
    rp2, ci2, _ = A2.export_csr()
    _bfs_check(A2, n, rp2.astype(np.int64), ci2.astype(np.int64), 3, "from_cplan")
    _bfs_check(pkg.Tiled.from_cplan(p, transpose=True), n, *mr.transpose_csr(n, n, rp2, ci2, np.zeros(len(ci2)))[:2], 3, "from_cplan^T")


# ---- the loops of INTEGRATION.md section 3p ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("rand_300", "band_1500"))
def test_torch_bfs_loop_equals_the_model(pkg, tctx, name):
    A, n, _, (rp, ci, v) = _operand(pkg, tctx, name, np.float64)
    src = 5
    level = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    level[src] = 0
    visited = torch.zeros(n, dtype=torch.bool, device="cuda")
    visited[src] = True
    frontier, nxt = visited.clone(), torch.zeros(n, dtype=torch.bool, device="cuda")
    count = torch.empty(n, dtype=torch.float64, device="cuda")
    depth = 0
    while True:
        A.mxv_frontier(None, frontier, visited, True, "plus_pair", True, out=count, out_present=nxt)
        if not bool(nxt.any()):
            break
        depth += 1
        level[nxt] = depth
        visited |= nxt
        frontier, nxt = nxt, frontier
    want, wdepth, _ = fr.bfs(n, rp, ci, src)
    assert np.array_equal(_host(level), want) and depth == wdepth
    assert np.array_equal(_host(A.bfs(src)[0]), want)


@pytest.mark.parametrize("name", ("rand_300", "band_1500"))
def test_torch_bellman_ford_loop_equals_the_model(pkg, tctx, name):
    """single-source shortest paths, edge i -> j of length |a_ij| + 0.1: every sweep relaxes only the edges out of the vertices whose
    distance changed in the last one (x_present), and equals the host loop over the model sweep by sweep; the end equals the plain
    sweeps over every edge (a vertex that did not change has nothing new to offer: its edges were relaxed with the same distance
    the sweep after it last changed)"""
    rows, cols, I, J, V, _ = CASES[name]
    n = rows
    rp, ci, v = _coo_csr(n, I, J, np.abs(np.asarray(V, np.float64)) + 0.1)
    A = pkg.Tiled.from_coo(tctx, n, n, np.repeat(np.arange(n, dtype=np.int32), np.diff(rp)), ci.astype(np.int32), v)
    src = 2
    d = np.full(n, np.inf)
    d[src] = 0.0
    changed = np.zeros(n, bool)
    changed[src] = True
    dd, dchanged = _dev(d), _dev(changed)
    t = torch.empty(n, dtype=torch.float64, device="cuda")
    sweeps = 0
    while changed.any():
        A.mxv_frontier(dd, dchanged, semiring="min_plus", transpose=True, out=t)
        new = torch.minimum(dd, t)
        dchanged = new < dd
        dd = new
        th, _ = fr.mxv_frontier(n, n, rp, ci, v, d, "min_plus", np.float64, changed, transpose=True)
        hnew = np.minimum(d, th)
        changed, d = hnew < d, hnew
        sweeps += 1
        assert np.array_equal(_host(dd), d) and np.array_equal(_host(dchanged), changed), f"sweep {sweeps}"
        assert sweeps <= n
    full = np.full(n, np.inf)
    full[src] = 0.0
    for _ in range(sweeps):
        full = np.minimum(full, mr.mxv(n, n, rp, ci, v, full, "min_plus", np.float64, transpose=True))
    assert np.array_equal(full, d) and sweeps > 2
