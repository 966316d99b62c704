"""GPU: arg folds of tilings (pem_tiled_mxv_arg / pem_tiled_reduce_arg / pem_tiled_bfs_parents).

The central check: A.mxv_arg equals argref's model -- the values by the `_same` rule of test_gpu_frontier.py, the index and the
presence bytes exactly -- while A's values and x are drawn from {-1, -0.0, 0.0, 1, 2, inf, -inf, nan} plus a few random ones, so
most rows have several equal best terms in different tiles: a walk that reports any attaining index, or the last one, fails.  The
absent x positions hold NaN and +-inf, idx holds a poison value that must survive wherever the contract says nothing is written.

Coverage.  Every case runs both orientations in fp64 and fp32 over fourteen (presence, mask, complement) combinations -- the dense
call (no presence bytes, no mask), the presences none / all / one / half / fiftieth without a mask, the masks on / off / half with
and without complement under a random half of x, a sparse-with-sparse pair and a dense x with a mask -- and all five kinds on every
combination; accumulate alternates over (combination, kind), so every kind sees both values in every case.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import argref as ar
import frontierref as fr
import mxvref as mr
from matgen import cases

pytestmark = pytest.mark.gpu

torch.cuda.is_available()   # (torch's runtime first, as in the other GPU files)

CASES = cases()
PEM_E_INVALID = -1
DTYPES = (np.float64, np.float32)
TIE = np.array([-1.0, -0.0, 0.0, 1.0, 2.0, np.inf, -np.inf, np.nan])
MINMAX = ar.VALUE_KINDS
POISON = np.array([np.nan, np.inf, -np.inf])
IDX_POISON = 7777777

# (case, the tiling built with transpose = 1)
TILINGS = [(n, False) for n in ("one_entry", "ragged_37", "dense_tile", "rect_33x65_AAt", "empty_rows", "empty_matrix", "powerlaw_600",
                                "hub_row_4000")] + [("rect_33x65_AAt", True)]
COMBOS = ([(None, None, False)] + [(p, None, False) for p in ("none", "all", "one", "half", "fiftieth")]
          + [("half", m, c) for m in ("on", "off", "half") for c in (False, True)] + [("fiftieth", "half", True), (None, "half", False)])


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


def _ties(n, seed, dtype):
    """values drawn to tie: the eight specials, and a random one in eight"""
    rng = np.random.default_rng(seed)
    v = rng.choice(TIE, n)
    r = rng.random(n) < 0.125
    v[r] = rng.standard_normal(int(r.sum()))
    return v.astype(dtype)


def _coo_csr(rows, I, J, V):
    I, J = np.asarray(I, np.int64), np.asarray(J, np.int64)
    o = np.lexsort((J, I))
    rp = np.zeros(rows + 1, np.int64)
    np.cumsum(np.bincount(I, minlength=rows), out=rp[1:])
    return rp, J[o], np.asarray(V)[o]


def _operand(pkg, ctx, name, dtype, transposed=False, ties=True):
    """(tiling, rows, cols, csr) of the matrix the tiling represents"""
    rows, cols, I, J, V, _ = CASES[name]
    W = _ties(len(V), rows * 7 + cols, dtype) if ties else np.asarray(V, dtype)
    rp, ci, v = _coo_csr(rows, I, J, W)
    Is = np.repeat(np.arange(rows, dtype=np.int32), np.diff(rp))
    A = pkg.Tiled.from_coo(ctx, rows, cols, Is, np.asarray(ci, np.int32), v, bool(transposed), dtype=dtype)
    if transposed:
        return A, cols, rows, mr.transpose_csr(rows, cols, rp, ci, v)
    return A, rows, cols, (rp, ci, v)


def _presence(kind, n, rng):
    if kind is None:
        return None
    p = np.zeros(n, bool)
    if kind == "all":
        p[:] = True
    elif kind == "one":
        p[n // 3] = True
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
    elif kind == "half":
        m = rng.random(n) < 0.5
    return m


def _poisoned(x, present):
    """x with NaN, +inf, -inf at the absent positions"""
    if present is None:
        return x
    x = x.copy()
    absent = np.flatnonzero(~present)
    x[absent] = POISON[np.arange(len(absent)) % 3]
    return x


def _bytes_dev(b, k):
    """the byte array as torch.bool or, every other time, as torch.uint8 holding 0 / 255 (any nonzero byte is on)"""
    if b is None:
        return None
    return _dev(b) if k % 2 == 0 else _dev(b.astype(np.uint8) * 255)


# ---- every case, dtype, orientation, kind, presence, mask ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name,transposed", TILINGS, ids=[n + ("^T" if t else "") for n, t in TILINGS])
def test_every_case_against_the_model(pkg, tctx, name, transposed, dtype):
    A, rows, cols, (rp, ci, v) = _operand(pkg, tctx, name, dtype, transposed)
    rng = np.random.default_rng(rows + 3 * cols)
    seen = set()
    for tr in (False, True):
        nx, ny = (rows, cols) if tr else (cols, rows)
        x0, y_old = _ties(nx, 11 + tr, dtype), _ties(ny, 13 + tr, dtype)
        # the old index of the index kinds: absent (-1, another negative) or some index that takes part
        i_old = np.where(rng.random(ny) < 0.5, rng.integers(0, max(nx, 1), ny), rng.integers(-3, 0, ny)).astype(np.int32)
        for c, (pk, mk, comp) in enumerate(COMBOS):
            present, mask = _presence(pk, nx, rng), _mask(mk, ny, rng)
            x = _poisoned(x0, present)
            dx, dp, dm = _dev(x), _bytes_dev(present, c), _bytes_dev(mask, c + 1)
            allowed = fr.allowed_of(ny, mask, comp)
            for k, kind in enumerate(ar.KINDS):
                acc = bool((c + k) % 2)
                seen.add((kind, acc))
                values = kind in ar.VALUE_KINDS
                label = f"{name} {kind} transpose={tr} present={pk} mask={mk} complement={comp} accumulate={acc}"
                idx_old = np.full(ny, IDX_POISON, np.int32) if values else i_old
                out = _dev(y_old) if values else None
                oidx, opres = _dev(idx_old), torch.full((ny,), 7, dtype=torch.uint8, device="cuda")
                r = A.mxv_arg(dx if values else None, kind, tr, dp, dm, comp, out, oidx, opres, acc)
                assert r[0] is out and r[1] is oidx
                gidx, gpres = _host(oidx), _host(opres)
                want, widx, wpres = ar.mxv_arg(rows, cols, rp, ci, v, x, kind, dtype, present, mask, comp, y_old, idx_old, acc, tr)
                assert np.array_equal(gidx, widx), f"{label}: idx at {np.flatnonzero(gidx != widx)[:5]}"
                assert np.array_equal(gpres, wpres), f"{label}: out_present"
                if values:
                    got = _host(out)
                    assert _same(got, want, kind), label
                    assert np.array_equal(_bits(got)[~allowed], _bits(y_old)[~allowed]), f"{label}: a disallowed output was written"
                    # the value is mxv_frontier's under the semiring of the same name
                    fy = _host(A.mxv_frontier(dx, dp, dm, comp, kind, tr, _dev(y_old), acc))
                    assert _same(got, fy, kind), f"{label}: differs from mxv_frontier"
                assert np.array_equal(gidx[~allowed], idx_old[~allowed]), f"{label}: idx of a disallowed output was written"
    assert len(seen) == 10   # every kind with both accumulate values


# ---- constructed rows: where the best sits, and what ties do --------------------------------------------------------------------------
N_LONG = 3300
LONG_COLS = np.array([16 * (15 * t) + c for t in range(1, 14) for c in range(16)][:200], np.int32)   # 13 tiles, 4 chunks of <= 64


def _long(pkg, ctx, vals, column, dtype):
    """the 1 x 3300 tiling whose row stores vals at LONG_COLS, or the 3300 x 1 tiling with them in its one column; its transpose flag"""
    z = np.zeros(len(LONG_COLS), np.int32)
    if column:
        return pkg.Tiled.from_coo(ctx, N_LONG, 1, LONG_COLS, z, np.asarray(vals, dtype), dtype=dtype), True
    return pkg.Tiled.from_coo(ctx, 1, N_LONG, z, LONG_COLS, np.asarray(vals, dtype), dtype=dtype), False


def _one(A, tr, kind, x=None, y_old=None, idx_old=IDX_POISON, acc=False, mask=None, dtype=np.float64):
    """(y, idx, present) of the single output"""
    values = kind in ar.VALUE_KINDS
    dx = _dev(np.zeros(N_LONG, dtype) if x is None else np.asarray(x, dtype)) if values else None
    out = _dev(np.array([np.nan if y_old is None else y_old], dtype)) if values else None
    oidx = _dev(np.array([idx_old], np.int32))
    opres = torch.full((1,), 9, dtype=torch.uint8, device="cuda")
    A.mxv_arg(dx, kind, tr, None, None if mask is None else _dev(np.array([mask])), False, out, oidx, opres, acc)
    return (float(_host(out)[0]) if values else None), int(_host(oidx)[0]), int(_host(opres)[0])


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("column", (False, True), ids=("row", "column"))
def test_constructed_long_line(pkg, tctx, column, dtype):
    n = len(LONG_COLS)
    first, last = int(LONG_COLS[0]), int(LONG_COLS[-1])
    kw = dict(dtype=dtype)
    # 200 equal values over 13 tiles and 4 chunks: the first index, the last for max_index
    A, tr = _long(pkg, tctx, np.ones(n), column, dtype)
    assert A.ntiles == 13
    assert _one(A, tr, "min_plus", **kw) == (1.0, first, 1)
    assert _one(A, tr, "max_plus", **kw) == (1.0, first, 1)
    assert _one(A, tr, "max_times", x=np.full(N_LONG, 2.0), **kw) == (2.0, first, 1)
    assert _one(A, tr, "min_index", **kw) == (None, first, 1)
    assert _one(A, tr, "max_index", **kw) == (None, last, 1)
    # accumulate: an old index below (above) every entering one stays, one inside the range loses; a negative one does not take part
    assert first == 240 and last == 3127
    assert _one(A, tr, "min_index", idx_old=3, acc=True, **kw)[1] == 3
    assert _one(A, tr, "min_index", idx_old=1000, acc=True, **kw)[1] == first
    assert _one(A, tr, "max_index", idx_old=3299, acc=True, **kw)[1] == 3299
    assert _one(A, tr, "max_index", idx_old=-5, acc=True, **kw)[1] == last
    # an old y equal to the best term: no term wins, idx untouched; an old y of NaN: the term wins
    assert _one(A, tr, "min_plus", y_old=1.0, acc=True, **kw) == (1.0, IDX_POISON, 1)
    assert _one(A, tr, "max_plus", y_old=1.0, acc=True, **kw) == (1.0, IDX_POISON, 1)
    assert _one(A, tr, "min_plus", y_old=np.nan, acc=True, **kw) == (1.0, first, 1)
    assert _one(A, tr, "max_times", x=np.ones(N_LONG), y_old=np.nan, acc=True, **kw) == (1.0, first, 1)
    assert _one(A, tr, "min_plus", y_old=1.5, acc=True, **kw) == (1.0, first, 1)
    assert _one(A, tr, "min_plus", y_old=0.5, acc=True, **kw) == (0.5, IDX_POISON, 1)
    # a disallowed output: y and the poison in idx survive, present is 0
    y, i, p = _one(A, tr, "min_plus", y_old=-3.0, mask=False, **kw)
    assert (y, i, p) == (-3.0, IDX_POISON, 0)
    assert _one(A, tr, "max_index", mask=False, **kw)[1:] == (IDX_POISON, 0)
    # the unique best in the first chunk, in the last, and as the very last entry; ties between chunk 1 and chunk 3
    for kind, best, rest in (("min_plus", -2.0, 1.0), ("max_plus", 5.0, 1.0), ("max_times", 5.0, 1.0)):
        x = np.ones(N_LONG) if kind == "max_times" else None
        for at in ((10,), (195,), (199,), (5, 140), (70, 195), (63, 64), (0, 199)):
            vals = np.full(n, rest)
            vals[list(at)] = best
            A, tr = _long(pkg, tctx, vals, column, dtype)
            assert _one(A, tr, kind, x=x, **kw) == (best, int(LONG_COLS[at[0]]), 1), (kind, at)
    # +0 and -0 tie: the lower index, whichever zero it holds
    vals = np.full(n, 1.0)
    vals[150], vals[20] = 0.0, -0.0
    A, tr = _long(pkg, tctx, vals, column, dtype)
    y, i, _ = _one(A, tr, "min_plus", **kw)
    assert y == 0.0 and i == int(LONG_COLS[20])
    vals[150], vals[20] = -0.0, 0.0
    A, tr = _long(pkg, tctx, vals, column, dtype)
    assert _one(A, tr, "min_plus", **kw)[1] == int(LONG_COLS[20])
    # an all-NaN row: -1 and the start value; present all the same (structural); with accumulate nothing moves
    A, tr = _long(pkg, tctx, np.full(n, np.nan), column, dtype)
    assert _one(A, tr, "min_plus", **kw) == (np.inf, -1, 1)
    assert _one(A, tr, "max_plus", **kw) == (-np.inf, -1, 1)
    assert _one(A, tr, "max_times", x=np.ones(N_LONG), **kw) == (-np.inf, -1, 1)
    assert _one(A, tr, "min_plus", y_old=4.0, acc=True, **kw) == (4.0, IDX_POISON, 1)
    assert _one(A, tr, "min_index", **kw) == (None, first, 1)   # NaN is an entry like any other
    # an infinite best is a term like any other: +inf wins a fresh min fold, and reports its first index
    vals = np.full(n, np.nan)
    vals[[77, 130]] = np.inf
    A, tr = _long(pkg, tctx, vals, column, dtype)
    assert _one(A, tr, "min_plus", **kw) == (np.inf, int(LONG_COLS[77]), 1)
    assert _one(A, tr, "min_plus", y_old=np.inf, acc=True, **kw) == (np.inf, IDX_POISON, 1)


# ---- reduce_arg ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name,transposed", TILINGS, ids=[n + ("^T" if t else "") for n, t in TILINGS])
def test_reduce_arg(pkg, tctx, name, transposed, dtype):
    A, rows, cols, (rp, ci, v) = _operand(pkg, tctx, name, dtype, transposed)
    for dim in ("rows", "cols"):
        for op in ("min", "max"):
            y, idx = A.reduce_arg(op, dim)
            assert idx.dtype == torch.int32
            wy, widx = ar.reduce_arg(rows, cols, rp, ci, v, op, dtype, dim)
            kind = op + "_plus"
            got = _host(y)
            assert _same(got, wy, kind) and np.array_equal(_host(idx), widx), f"{name} {op} {dim}"
            assert _same(got, _host(A.reduce(op, dim)), kind), f"{name} {op} {dim}: differs from reduce"
            # the same through mxv_arg with a zero x
            n = rows if dim == "cols" else cols
            zy, zidx = A.mxv_arg(torch.zeros(n, dtype=y.dtype, device="cuda"), kind, dim == "cols")
            assert _same(got, _host(zy), kind) and np.array_equal(_host(idx), _host(zidx)), f"{name} {op} {dim}: differs from mxv_arg(x = 0)"


# ---- bfs_parents -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("powerlaw_600", "banded_500_AAt", "empty_rows", "diag_100"))
def test_bfs_parents_against_the_model(pkg, tctx, name):
    A, n, _, (rp, ci, v) = _operand(pkg, tctx, name, np.float64)   # (the values include explicit zeros and NaN: they are edges)
    deg = np.diff(rp)
    if name == "empty_rows":
        sources = [int(np.flatnonzero(deg == 0)[0]), 0]
    elif name == "diag_100":
        sources = [41]
    else:
        sources = [0, int(np.argmax(deg))]
    several = 0
    for src in sources:
        for tr in (False, True):
            label = f"{name} from {src} transpose={tr}"
            lv, par, depth, reached = A.bfs_parents(src, transpose=tr)
            blv, bdepth, breached = A.bfs(src, transpose=tr)
            wl, wp, wd, wr = ar.bfs_parents(n, rp, ci, src, tr)
            assert lv.dtype == torch.int32 and par.dtype == torch.int32
            assert np.array_equal(_host(lv), _host(blv)) and (depth, reached) == (bdepth, breached), f"{label}: differs from bfs"
            assert np.array_equal(_host(lv), wl) and (depth, reached) == (wd, wr), f"{label}: levels"
            assert np.array_equal(_host(par), wp), f"{label}: parents"
            several += int((ar.candidate_parents(n, rp, ci, wl, tr)[wl > 0] > 1).sum())
    if name == "diag_100":
        assert (wd, wr) == (0, 1)
    if name == "empty_rows":
        assert (wl < 0).any()
    if name in ("powerlaw_600", "banded_500_AAt"):
        assert several > 0, "no vertex has two candidate parents: the least-parent rule is not exercised"


def test_bfs_parents_on_an_fp32_tiling(pkg, tctx):
    F, n, _, (rp, ci, v) = _operand(pkg, tctx, "powerlaw_600", np.float32)
    lv, par, depth, reached = F.bfs_parents(7)
    wl, wp, wd, wr = ar.bfs_parents(n, rp, ci, 7)
    assert np.array_equal(_host(lv), wl) and np.array_equal(_host(par), wp) and (depth, reached) == (wd, wr)


# ---- determinism, allocations ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("powerlaw_600", "hub_row_4000"))
def test_two_calls_identical_and_second_call_allocates_nothing(pkg, tctx, name):
    A, rows, cols, _ = _operand(pkg, tctx, name, np.float64)
    rng = np.random.default_rng(2)
    for tr in (False, True):
        nx, ny = (rows, cols) if tr else (cols, rows)
        present, mask = _dev(_presence("half", nx, rng)), _dev(_mask("half", ny, rng))
        x = _dev(_ties(nx, 3, np.float64))
        for kind in ar.KINDS:
            values = kind in ar.VALUE_KINDS
            runs = []
            for rep in range(2):
                if rep == 1:
                    before = tctx.memory_stats()["block_allocs"]
                out = torch.zeros(ny, dtype=torch.float64, device="cuda") if values else None
                oidx = torch.full((ny,), -1, dtype=torch.int32, device="cuda")
                op = torch.zeros(ny, dtype=torch.uint8, device="cuda")
                A.mxv_arg(x if values else None, kind, tr, present, mask, True, out, oidx, op)
                runs.append((_host(out).tobytes() if values else b"", _host(oidx).tobytes(), _host(op).tobytes()))
            assert tctx.memory_stats()["block_allocs"] == before, f"{name} {kind} transpose={tr}: a repeat call allocated"
            assert runs[0] == runs[1], f"{name} {kind} transpose={tr}: two calls differ"
        r1, r2 = A.reduce_arg("max", "cols" if tr else "rows"), A.reduce_arg("max", "cols" if tr else "rows")
        assert _host(r1[0]).tobytes() == _host(r2[0]).tobytes() and _host(r1[1]).tobytes() == _host(r2[1]).tobytes()
    p1, p2 = A.bfs_parents(0), A.bfs_parents(0)
    assert _host(p1[1]).tobytes() == _host(p2[1]).tobytes() and _host(p1[0]).tobytes() == _host(p2[0]).tobytes()


def test_empty_tiling_and_zero_length(pkg, tctx):
    rows, cols, I, J, V, _ = CASES["empty_matrix"]
    E = pkg.Tiled.from_coo(tctx, rows, cols, I, J, V)
    for kind in ar.KINDS:
        values = kind in ar.VALUE_KINDS
        for tr in (False, True):
            y, idx = E.mxv_arg(_dev(np.ones(cols)) if values else None, kind, tr, _dev(np.ones(cols, bool)))
            assert np.array_equal(_host(idx), np.full(rows, -1, np.int32)), kind
            if values:
                assert _same(_host(y), np.full(rows, ar.START[kind])), kind
            oidx = _dev(np.full(rows, IDX_POISON, np.int32))
            E.mxv_arg(_dev(np.ones(cols)) if values else None, kind, tr, out_index=oidx, accumulate=True)
            assert np.array_equal(_host(oidx), np.full(rows, IDX_POISON, np.int32)), kind


# ---- errors ------------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments(pkg, tctx):
    L = pkg.lib()
    A, rows, cols, _ = _operand(pkg, tctx, "rect_33x65_AAt", np.float64)
    F, _, _, _ = _operand(pkg, tctx, "rect_33x65_AAt", np.float32)
    S, n, _, _ = _operand(pkg, tctx, "ragged_37", np.float64)
    x, y = _dev(np.ones(cols)), _dev(np.zeros(rows))
    xf, yf = _dev(np.ones(cols, np.float32)), _dev(np.zeros(rows, np.float32))
    xp, m, yp = _dev(np.ones(cols, bool)), _dev(np.ones(rows, bool)), _dev(np.zeros(rows, np.uint8))
    ix = _dev(np.zeros(rows, np.int32))
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    fx, f32 = L.pem_tiled_mxv_arg, L.pem_tiled_mxv_arg_f32

    def call(ctx=tctx._h, a=A._h, k=0, tr=0, dx=P(x), dxp=P(xp), dy=P(y), di=P(ix), dm=P(m), comp=0, dyp=P(yp), acc=0, fn=fx):
        return fn(ctx, a, k, tr, dx, dxp, dy, di, dm, comp, dyp, acc)

    assert call() == 0
    assert call(k=3, dx=None, dy=None) == 0 and call(k=4, dx=None, dy=None) == 0   # the index kinds read no value
    assert call(dxp=None, dm=None, dyp=None) == 0
    tctx.synchronize()
    before = tctx.memory_stats()
    bad = [call(ctx=None), call(a=None), call(dx=None), call(dy=None), call(di=None), call(k=3, di=None), call(k=5), call(k=-1),
           call(tr=2), call(tr=-1), call(acc=2), call(comp=2), call(comp=-1),
           call(fn=f32, dx=P(xf), dy=P(yf)),       # fp64 tiling, fp32 entry
           call(a=F._h), call(a=F._h, k=3)]        # fp32 tiling, fp64 entry
    assert bad == [PEM_E_INVALID] * len(bad)
    # overlaps: the frontier's (out_present with the mask, x_present, x and y; x with y) ...
    both = _dev(np.ones(2 * rows + cols, np.uint8))
    b0 = both.data_ptr()
    assert call(dm=C.c_void_p(b0), dyp=C.c_void_p(b0 + rows - 1)) == PEM_E_INVALID
    assert call(dxp=C.c_void_p(b0), dyp=C.c_void_p(b0 + cols - 1)) == PEM_E_INVALID
    assert call(dyp=C.c_void_p(x.data_ptr() + 8 * cols - 1)) == PEM_E_INVALID
    assert call(dyp=C.c_void_p(y.data_ptr())) == PEM_E_INVALID
    buf = _dev(np.ones(cols + rows))
    p0 = buf.data_ptr()
    assert call(dx=C.c_void_p(p0), dy=C.c_void_p(p0 + 8 * (cols - 1))) == PEM_E_INVALID
    # ... and d_idx with every other argument
    big = _dev(np.zeros(4 * rows + 8 * cols, np.uint8))
    g0 = big.data_ptr()
    assert call(di=C.c_void_p(g0), dm=C.c_void_p(g0 + 4 * rows - 1)) == PEM_E_INVALID
    assert call(di=C.c_void_p(g0), dyp=C.c_void_p(g0 + 4 * rows - 1)) == PEM_E_INVALID
    assert call(di=C.c_void_p(g0), dxp=C.c_void_p(g0 + 4 * rows - 1)) == PEM_E_INVALID
    assert call(di=C.c_void_p(g0), dx=C.c_void_p(g0 + 4 * rows - 4)) == PEM_E_INVALID
    assert call(di=C.c_void_p(y.data_ptr() + 8 * rows - 4)) == PEM_E_INVALID
    assert call(di=C.c_void_p(y.data_ptr())) == PEM_E_INVALID
    # reduce_arg: ops without an arg, dims, types, nulls, overlap
    ra = lambda ctx=tctx._h, a=A._h, op=2, dim=0, dy=P(y), di=P(ix), fn=L.pem_tiled_reduce_arg: fn(ctx, a, op, dim, dy, di)
    bad = [ra(ctx=None), ra(a=None), ra(op=0), ra(op=1), ra(op=4), ra(op=-1), ra(dim=2), ra(dim=-1), ra(dy=None), ra(di=None), ra(a=F._h),
           ra(fn=L.pem_tiled_reduce_arg_f32, dy=P(yf)), ra(di=C.c_void_p(y.data_ptr() + 8))]
    assert bad == [PEM_E_INVALID] * len(bad)
    # bfs_parents: bfs's cases, a null or overlapping d_parent
    lv, pa = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    d, r = C.c_int32(), C.c_int64()
    bp = lambda ctx=tctx._h, a=S._h, src=0, tr=0, dl=P(lv), dp=P(pa), dd=C.byref(d), rr=C.byref(r): L.pem_tiled_bfs_parents(
        ctx, a, C.c_int64(src), tr, dl, dp, dd, rr)
    bad = [bp(ctx=None), bp(a=None), bp(a=A._h), bp(src=-1), bp(src=n), bp(tr=2), bp(dl=None), bp(dp=None), bp(dd=None), bp(rr=None),
           bp(dp=C.c_void_p(lv.data_ptr() + 4 * (n - 1)))]
    assert bad == [PEM_E_INVALID] * len(bad)
    assert tctx.memory_stats() == before, "a refused call touched the context's memory"
    # what is legal next to them: adjacent buffers
    assert call(dm=C.c_void_p(b0), dyp=C.c_void_p(b0 + rows)) == 0
    assert call(di=C.c_void_p(g0), dm=C.c_void_p(g0 + 4 * rows)) == 0
    assert call(k=3, di=C.c_void_p(y.data_ptr()), dx=None, dy=P(y)) == 0   # an index kind: dy is nobody's
    assert ra() == 0 and ra(op=3, dim=1, dy=P(_dev(np.zeros(cols))), di=P(_dev(np.zeros(cols, np.int32)))) == 0
    assert bp() == 0
    tctx.synchronize()
    # the Python layer
    with pytest.raises(ValueError, match="unknown kind"):
        A.mxv_arg(x, "plus_times")
    with pytest.raises(ValueError, match="want a contiguous device tensor"):
        A.mxv_arg(None, "min_plus")                # only the index kinds do without x
    with pytest.raises(ValueError, match="int32"):
        A.mxv_arg(x, "min_plus", out_index=_dev(np.zeros(rows, np.int64)))
    with pytest.raises(ValueError, match="int32"):
        A.mxv_arg(x, "min_plus", out_index=_dev(np.zeros(rows + 1, np.int32)))
    with pytest.raises(ValueError, match="writes no value"):
        A.mxv_arg(None, "min_index", out=y)
    with pytest.raises(ValueError, match="want a contiguous device tensor"):
        A.mxv_arg(x, "min_plus", x_present=_dev(np.ones(cols, np.int32)))
    with pytest.raises(ValueError):
        A.reduce_arg("plus")
    with pytest.raises(ValueError):
        A.reduce_arg("max", "diag")
    with pytest.raises(pkg.PemError):
        S.bfs_parents(n)
