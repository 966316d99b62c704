"""GPU: the Krylov solvers (pem_krylov_*).

x, iters, status and the written history of every solve equal krylovref bit for bit (NaN equal to NaN), for every case of
krylovcases x {cg where SPD, bicgstab} x {none, diag, LU} x {fp64, fp32}; the entries of the history past iters keep a poison
value.  fp64 solves stop at RTOL, fp32 ones at RTOL32 (fp32 residuals cannot reach 1e-8).  The references are computed once per
combination and shared.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ilu0ref as ir
import krylovcases as kc
import krylovref as kr
import trsvref as tr

pytestmark = pytest.mark.gpu

torch.cuda.is_available()   # (torch's runtime first, as in the other GPU files)

CASES = kc.cases()
PEM_E_INVALID = -1
POISON = -7.0
DT = {"f64": np.float64, "f32": np.float32}
COMBOS = [(name, m, pc, dt) for name, (_, spd) in CASES.items() for m in (("cg", "bicgstab") if spd else ("bicgstab",))
          for pc in ("none", "diag", "lu") for dt in DT]


@pytest.fixture(scope="module")
def tctx(pkg):
    """a context on a torch stream made current for the module: torch's work and the library's calls are ordered with no extra sync"""
    prev = torch.cuda.current_stream()
    s = torch.cuda.Stream()
    torch.cuda.set_stream(s)
    c = pkg.Context(0, stream=s.cuda_stream)
    yield c
    c.close()
    torch.cuda.set_stream(prev)


def _rtol(dtype):
    return kc.RTOL if np.dtype(dtype) == np.float64 else kc.RTOL32


@functools.lru_cache(maxsize=None)
def _system(name, dt):
    """(n, rp, ci, v, b, x0, minv, f): the case as CSR in the dtype, its right-hand side, inverse diagonal and ILU(0) values"""
    dtype = DT[dt]
    n, rp, ci, v = kc.csr(CASES[name][0], dtype)
    b, x0 = kc.rhs(name, n, dtype)
    I = np.repeat(np.arange(n), np.diff(rp))
    minv = (dtype(1) / v[I == ci]).astype(dtype)
    f, _ = ir.ilu0(n, rp, ci, v, dtype)
    return n, rp, ci, v, b, x0, minv, f


_ORACLE = []


@functools.lru_cache(maxsize=None)
def _ref(name, method, pc, dt, max_iters=kc.MAX_ITERS):
    n, rp, ci, v, b, x0, minv, f = _system(name, dt)
    return kr.solve(n, rp, ci, v, b, x0, method, pc, minv=minv, factor=(rp, ci, f), max_iters=max_iters, rtol=_rtol(DT[dt]), dtype=DT[dt],
                    oracle=_ORACLE[0])


@pytest.fixture(scope="module", autouse=True)
def _bind_oracle(oracle):
    _ORACLE[:] = [oracle]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    return bool(np.all((got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want))))


_TILINGS = {}


def _tilings(pkg, ctx, name, dt):
    """(A, F) of a case, built once"""
    if (name, dt) not in _TILINGS:
        n, rp, ci, v, *_ = _system(name, dt)
        I = np.repeat(np.arange(n, dtype=np.int32), np.diff(rp))
        A = pkg.Tiled.from_coo(ctx, n, n, I, np.asarray(ci, np.int32), v, dtype=DT[dt])
        _TILINGS[(name, dt)] = (A, A.ilu0())
    return _TILINGS[(name, dt)]


@pytest.fixture(scope="module", autouse=True)
def _drop_tilings():
    yield
    for A, F in _TILINGS.values():
        F.close()
        A.close()
    _TILINGS.clear()


def _trsv_launches(F):
    return F.trsv_info("lower")["launches"] + F.trsv_info("upper")["launches"]


def _run(pkg, ctx, name, method, pc, dt, check_every=8, max_iters=kc.MAX_ITERS, system=None, tilings=None):
    """one device solve -> (x, history (host, max_iters + 1 entries), info)"""
    n, rp, ci, v, b, x0, minv, f = system or _system(name, dt)
    A, F = tilings or _tilings(pkg, ctx, name, dt)
    K = pkg.Krylov(A, method=method, precond={"none": None, "diag": "diag", "lu": F}[pc], max_iters=max_iters, check_every=check_every,
                   rtol=_rtol(DT[dt]))
    hist = torch.full((max_iters + 1,), POISON, dtype=torch.float64, device="cuda")
    x, info = K.solve(_dev(b), x=_dev(x0), minv=_dev(minv) if pc == "diag" else None, history=hist)
    K.close()
    return x.cpu().numpy(), hist.cpu().numpy(), info


def _check(got, ref, method, pc, check_every, max_iters, T):
    x, hist, info = got
    k = ref["iters"]
    assert (info["iters"], info["status_code"]) == (k, ref["status"]), (info, kr.STATUS[ref["status"]], k)
    assert _same(x, ref["x"])
    assert _same(hist[:k + 1], ref["history"]) and np.all(hist[k + 1:] == POISON)
    assert _same(info["history"].cpu().numpy(), ref["history"])
    for key in ("bb", "rr", "threshold"):
        assert _same(np.float64(info[key]), np.float64(ref[key])), key
    assert info["readbacks"] == kr.readbacks(ref["stop_iter"], check_every)
    assert info["launches"] == kr.launches(method, pc, ref["stop_iter"], check_every, max_iters, T)


@pytest.mark.parametrize("name,method,pc,dt", COMBOS, ids=["-".join(c) for c in COMBOS])
def test_solve_matches_the_reference(pkg, tctx, name, method, pc, dt):
    ref = _ref(name, method, pc, dt)
    assert ref["status"] == kr.CONVERGED
    T = _trsv_launches(_tilings(pkg, tctx, name, dt)[1]) if pc == "lu" else 0
    _check(_run(pkg, tctx, name, method, pc, dt), ref, method, pc, 8, kc.MAX_ITERS, T)


EVERY = [("spd_grid_40x40_red_black", "cg", "lu", "f64"), ("gen_hubs_1600", "bicgstab", "diag", "f32"),
         ("spd_tridiagonal_4097", "cg", "none", "f64"), ("gen_grid_40x40_red_black", "bicgstab", "lu", "f64"),
         ("spd_dense_33", "bicgstab", "none", "f32")]


@pytest.mark.parametrize("name,method,pc,dt", EVERY, ids=["-".join(c) for c in EVERY])
def test_check_every_changes_no_bit(pkg, tctx, name, method, pc, dt):
    ref = _ref(name, method, pc, dt)
    T = _trsv_launches(_tilings(pkg, tctx, name, dt)[1]) if pc == "lu" else 0
    for ce in (1, 7, kc.MAX_ITERS):
        _check(_run(pkg, tctx, name, method, pc, dt, check_every=ce), ref, method, pc, ce, kc.MAX_ITERS, T)


def test_max_iters(pkg, tctx):
    for method in ("cg", "bicgstab"):
        for mi in (3, 0):
            ref = _ref("spd_tridiagonal_200", method, "diag", "f64", max_iters=mi)
            assert (ref["status"], ref["iters"]) == (kr.MAX_ITERS, mi)
            _check(_run(pkg, tctx, "spd_tridiagonal_200", method, "diag", "f64", max_iters=mi), ref, method, "diag", 8, mi, 0)


def _small(pkg, ctx, rows, b, x0, method, dt, max_iters=20):
    """a small dense system on the device and in the reference -> (got, ref)"""
    dtype = DT[dt]
    M = np.array(rows, float)
    n = len(M)
    I, J = np.nonzero(M)
    case = (n, I, J, M[I, J])
    n, rp, ci, v = kc.csr(case, dtype)
    system = (n, rp, ci, v, np.asarray(b, dtype), np.asarray(x0, dtype), None, None)
    A = pkg.Tiled.from_coo(ctx, n, n, I.astype(np.int32), J.astype(np.int32), M[I, J], dtype=dtype)
    try:
        got = _run(pkg, ctx, None, method, "none", dt, max_iters=max_iters, system=system, tilings=(A, None))
    finally:
        A.close()
    ref = kr.solve(n, rp, ci, v, system[4], system[5], method, max_iters=max_iters, rtol=_rtol(dtype), dtype=dtype, oracle=_ORACLE[0])
    return got, ref


@pytest.mark.parametrize("dt", list(DT))
def test_every_status_on_the_device(pkg, tctx, dt):
    # CG, indefinite: breakdown at k = 1, x stays the guess
    x0 = [0.5, 0.25]
    got, ref = _small(pkg, tctx, [[1, 0], [0, -1]], [1, 2], x0, "cg", dt)
    assert (ref["status"], ref["iters"], ref["reason"]) == (kr.BREAKDOWN, 0, "pq")
    _check(got, ref, "cg", "none", 8, 20, 0)
    assert _same(got[0], np.asarray(x0, DT[dt]))
    # BiCGStab, the rotation: rv = 0 at k = 1, x stays the guess
    got, ref = _small(pkg, tctx, [[0, -1], [1, 0]], [1, 0], [0, 0], "bicgstab", dt)
    assert (ref["status"], ref["iters"], ref["reason"]) == (kr.BREAKDOWN, 0, "rv")
    _check(got, ref, "bicgstab", "none", 8, 20, 0)
    assert _same(got[0], np.zeros(2, DT[dt]))
    # BiCGStab, rho' = 0 after the first iteration (test_krylov_cpu.py has the arithmetic)
    got, ref = _small(pkg, tctx, [[-1, -1, -1], [-1, -1, -1], [-1, 1, 0]], [0, 1, 0], [0, 0, 0], "bicgstab", dt)
    assert (ref["status"], ref["iters"], ref["reason"]) == (kr.BREAKDOWN, 1, "rho")
    _check(got, ref, "bicgstab", "none", 8, 20, 0)
    for method in ("cg", "bicgstab"):
        # b = 0 with a zero guess: converged at the start
        got, ref = _small(pkg, tctx, [[2, 1], [1, 3]], [0, 0], [0, 0], method, dt)
        assert (ref["status"], ref["iters"]) == (kr.CONVERGED, 0)
        _check(got, ref, method, "none", 8, 20, 0)
        # a NaN in b
        got, ref = _small(pkg, tctx, [[2, 1], [1, 3]], [np.nan, 1], [0.5, 0.5], method, dt)
        assert (ref["status"], ref["iters"]) == (kr.NONFINITE, 0)
        _check(got, ref, method, "none", 8, 20, 0)
        assert _same(got[0], np.asarray([0.5, 0.5], DT[dt]))


@pytest.mark.parametrize("method,dt", [("cg", "f64"), ("bicgstab", "f32")])
def test_new_values_need_nothing_rebuilt(pkg, tctx, method, dt):
    """a second solve, and a solve after A.set_values_device + F.set_values_from_ilu0, allocate nothing and match the reference"""
    name = "spd_grid_40x40_red_black"
    dtype = DT[dt]
    n, rp, ci, v, b, x0, minv, f = _system(name, dt)
    I = np.repeat(np.arange(n, dtype=np.int32), np.diff(rp))
    A = pkg.Tiled.from_coo(tctx, n, n, I, np.asarray(ci, np.int32), v, dtype=dtype)
    F = A.ilu0()
    K = pkg.Krylov(A, method=method, precond=F, max_iters=kc.MAX_ITERS, rtol=_rtol(dtype))
    db, dx = _dev(b), _dev(x0)
    v2 = (v * dtype(1.25)).astype(dtype)   # still symmetric and dominant
    dv, dv2 = _dev(v), _dev(v2)
    A.set_values_device(dv2)   # (the first refresh builds the value maps)
    F.set_values_from_ilu0(A)
    A.set_values_device(dv)
    F.set_values_from_ilu0(A)
    x, info = K.solve(db, x=dx)
    ref = _ref(name, method, "lu", dt)
    assert _same(x.cpu().numpy(), ref["x"]) and info["iters"] == ref["iters"]
    before = tctx.memory_stats()["block_allocs"]
    dx.copy_(_dev(x0))
    x, info = K.solve(db, x=dx)
    assert _same(x.cpu().numpy(), ref["x"])
    A.set_values_device(dv2)
    F.set_values_from_ilu0(A)
    dx.copy_(_dev(x0))
    x, info = K.solve(db, x=dx)
    assert tctx.memory_stats()["block_allocs"] == before
    f2, _ = ir.ilu0(n, rp, ci, v2, dtype)
    ref2 = kr.solve(n, rp, ci, v2, b, x0, method, "lu", factor=(rp, ci, f2), max_iters=kc.MAX_ITERS, rtol=_rtol(dtype), dtype=dtype,
                    oracle=_ORACLE[0])
    assert (info["iters"], info["status_code"]) == (ref2["iters"], ref2["status"]) and _same(x.cpu().numpy(), ref2["x"])
    K.close()
    F.close()
    A.close()


BUDGET = [("spd_grid_40x40_red_black", "cg", "none", 3), ("spd_grid_40x40_red_black", "cg", "diag", 3),
          ("spd_grid_40x40_red_black", "cg", "lu", 4), ("gen_hubs_1600", "bicgstab", "none", 5), ("gen_hubs_1600", "bicgstab", "diag", 5),
          ("gen_hubs_1600", "bicgstab", "lu", 5)]


@pytest.mark.parametrize("name,method,pc,budget", BUDGET, ids=["-".join(c[:3]) for c in BUDGET])
def test_launch_budget(pkg, tctx, name, method, pc, budget):
    """kernel_stats: the solver's own kernels per enqueued iteration stay within the header's budget, beside one mxv (CG) or two"""
    ref = _ref(name, method, pc, "f64")
    _tilings(pkg, tctx, name, "f64")
    tctx.synchronize()
    tctx.set_kernel_profiling(True)
    tctx.reset_kernel_stats()
    try:
        _, _, info = _run(pkg, tctx, name, method, pc, "f64", check_every=1)
        tctx.synchronize()
        stats = tctx.kernel_stats()
    finally:
        tctx.set_kernel_profiling(False)
    E = info["readbacks"]   # check_every = 1: the iterations enqueued
    assert E == ref["stop_iter"]
    own = {k: s["calls"] for k, s in stats.items() if k.startswith("krylov_")}
    mxv = sum(s["calls"] for k, s in stats.items() if k.startswith("mxv_kernel"))
    start = (3 if pc == "lu" else 2) if method == "cg" else 2
    assert sum(own.values()) == start + budget * E, own
    assert mxv == 1 + (1 if method == "cg" else 2) * E
    if method == "cg":
        assert own == {"krylov_init": 1, "krylov_cg_p": E + 1, "krylov_cg_update": E, "krylov_dot": (2 * E + 1) if pc == "lu" else E}
    else:
        assert own == {"krylov_init": 1, "krylov_bi_p": E + 1, "krylov_dot": E, "krylov_bi_s": E, "krylov_bi_ts": E, "krylov_bi_xr": E}


@pytest.mark.parametrize("n", [1, 255, 257, 4095, 4096, 4097, 4096 * 1024 + 1])
def test_dot_hook_is_bit_exact(pkg, tctx, n):
    """the partition's edges: below a wave, around a workgroup, around a chunk, and the wrap of the chunk loop (chunk 1024 goes to
    workgroup 0 again)"""
    rng = np.random.default_rng(n)
    for dtype in DT.values():
        u, v = rng.standard_normal(n).astype(dtype), rng.standard_normal(n).astype(dtype)
        got = pkg.krylov_dot(tctx, _dev(u), _dev(v))
        assert _same(np.float64(got), kr.dot(u, v)), (n, dtype)


def test_refusals(pkg, tctx):
    lib = pkg.lib()
    A, F = _tilings(pkg, tctx, "spd_dense_17", "f64")
    A32, F32 = _tilings(pkg, tctx, "spd_dense_17", "f32")
    B, _ = _tilings(pkg, tctx, "spd_dense_15", "f64")
    R = pkg.Tiled.from_coo(tctx, 3, 4, [0, 1], [1, 2], [1.0, 2.0])
    n = A.rows

    def create(A_, method=0, precond=0, F_=None, max_iters=10, check_every=1, rtol=1e-8, atol=0.0, opts=True, out=True, ctx=True):
        o = pkg.KrylovOpts(method, precond, max_iters, check_every, rtol, atol)
        h = C.c_void_p(1)
        st = lib.pem_krylov_create(tctx._h if ctx else None, A_._h if A_ is not None else None, C.byref(o) if opts else None,
                                   F_._h if F_ is not None else None, C.byref(h) if out else None)
        if st == 0:
            lib.pem_krylov_destroy(tctx._h, h)
        else:
            assert not out or not h.value
        return st

    assert create(A) == 0 and create(A, 1, 2, F) == 0
    for kw in (dict(ctx=False), dict(A_=None), dict(opts=False), dict(out=False), dict(A_=R), dict(method=2), dict(method=-1),
               dict(precond=3), dict(precond=-1), dict(precond=2), dict(precond=0, F_=F), dict(precond=1, F_=F), dict(precond=2, F_=B),
               dict(precond=2, F_=F32), dict(max_iters=-1), dict(check_every=0), dict(rtol=-1.0), dict(rtol=float("nan")),
               dict(atol=-1.0), dict(atol=float("nan"))):
        kw.setdefault("A_", A)
        assert create(**kw) == PEM_E_INVALID, kw
        assert b"pem_krylov_create" in lib.pem_last_error()
    # a factor without a stored diagonal: trsv's message
    i, j = np.tril_indices(5, -1)
    L = pkg.Tiled.from_coo(tctx, 5, 5, i.astype(np.int32), j.astype(np.int32), np.ones(len(i)))
    S = pkg.Tiled.from_coo(tctx, 5, 5, np.arange(5, dtype=np.int32), np.arange(5, dtype=np.int32), np.ones(5))
    with pytest.raises(pkg.PemError, match="no stored diagonal entry") as e:
        pkg.Krylov(S, precond=L)
    assert e.value.status == PEM_E_INVALID
    # solve
    K = pkg.Krylov(A, precond="diag", max_iters=10)
    K32 = pkg.Krylov(A32, max_iters=10)
    buf = torch.zeros(4 * n + 16, dtype=torch.float64, device="cuda")
    b, x, m, h = buf[:n], buf[n:2 * n], buf[2 * n:3 * n], buf[3 * n:3 * n + 11]
    res = pkg.KrylovResult()

    def solve(K_, b_, x_, m_, h_, res_=True, fn=lib.pem_krylov_solve, ctx=True):
        p = [C.c_void_p(t.data_ptr()) if t is not None else None for t in (b_, x_, m_, h_)]
        return fn(tctx._h if ctx else None, K_._h if K_ is not None else None, *p, C.byref(res) if res_ else None)

    m.fill_(1.0)
    torch.cuda.current_stream().synchronize()
    assert solve(K, b, x, m, h) == 0 and res.status == 0 and res.iters == 0
    for args, kw in (((K, b, x, m, h), dict(ctx=False)), ((None, b, x, m, h), {}), ((K, b, x, m, h), dict(res_=False)),
                     ((K, b, x, m, h), dict(fn=lib.pem_krylov_solve_f32)), ((K32, b, x, None, h), {}), ((K, None, x, m, h), {}),
                     ((K, b, None, m, h), {}), ((K, b, x, None, h), {}), ((K, b, b, m, h), {}), ((K, b, buf[n - 1:2 * n - 1], m, h), {}),
                     ((K, b, x, b, h), {}), ((K, b, x, x, h), {}), ((K, b, x, m, buf[3 * n - 1:]), {}), ((K, b, x, m, buf[:11]), {}),
                     ((K, b, x, m, buf[2 * n - 5:]), {})):
        assert solve(*args, **kw) == PEM_E_INVALID, (args[1:], kw)
        assert b"pem_krylov_solve" in lib.pem_last_error()
    # the Python argument checks
    tb = torch.zeros(n, dtype=torch.float64, device="cuda")
    for bad in (lambda: pkg.Krylov(A, method="gmres"), lambda: pkg.Krylov(A, precond="ilu"), lambda: pkg.Krylov(A, max_iters=1.5),
                lambda: pkg.Krylov(A, check_every=True), lambda: pkg.Krylov(A, rtol="x"), lambda: K.solve(tb),
                lambda: K32.solve(tb), lambda: K.solve(tb[:-1], minv=tb), lambda: K.solve(tb.cpu(), minv=tb),
                lambda: K32.solve(tb.float(), minv=tb.float()), lambda: K.solve(tb, minv=tb, history=torch.zeros(3, device="cuda")),
                lambda: A.solve(tb, precond="ssor")):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(pkg.PemError):
        pkg.Krylov(R)
    K.close()
    K32.close()
    for t in (R, L, S):
        t.close()


@pytest.mark.parametrize("dt", list(DT))
def test_one_shot_and_torch_reads_x_without_a_sync(pkg, tctx, dt):
    """Tiled.solve with "jacobi" and "ilu0" equals the solver object with the same preconditioner; torch reads x on its stream (the
    context's) straight after the call"""
    name = "spd_hubs_1600"
    dtype = DT[dt]
    n, rp, ci, v, b, x0, minv, f = _system(name, dt)
    A, F = _tilings(pkg, tctx, name, dt)
    db = _dev(b)
    x, info = A.solve(db, method="cg", precond="ilu0", x=_dev(x0), max_iters=kc.MAX_ITERS, rtol=_rtol(dtype), history=True)
    got = (x * 1).cpu().numpy()   # torch's kernel and copy, ordered behind the solve
    ref = _ref(name, "cg", "lu", dt)
    assert _same(got, ref["x"]) and info["status"] == "converged" and info["rnorm"] == np.sqrt(ref["rr"])
    assert _same(info["history"].cpu().numpy(), ref["history"])
    x, info = A.solve(db, method="bicgstab", precond="jacobi", x=_dev(x0), max_iters=kc.MAX_ITERS, rtol=_rtol(dtype))
    ref = _ref(name, "bicgstab", "diag", dt)
    assert _same(x.cpu().numpy(), ref["x"]) and info["iters"] == ref["iters"]
    # a zero guess by default
    x, info = A.solve(db, rtol=_rtol(dtype))
    r = kr.solve(n, rp, ci, v, b, np.zeros(n, dtype), "cg", max_iters=1000, rtol=_rtol(dtype), dtype=dtype, oracle=_ORACLE[0])
    assert _same(x.cpu().numpy(), r["x"]) and info["iters"] == r["iters"]
