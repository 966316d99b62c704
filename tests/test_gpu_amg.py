"""GPU: the aggregation multigrid (pem_amg_*, pem_krylov_create_amg).

Every level of every hierarchy (A_l, P_l, R_l as exported CSR), the info, one V-cycle and the preconditioned solves equal the host
model amgref bit for bit (NaN equal to NaN), over amgcases' cases and option grid, fp64 and fp32; on three cases the levels also
equal what the public calls give through the binding.  The references are computed once per combination and shared.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import aggref
import amgcases as ac
import amgref as ar
import krylovref as kr

pytestmark = pytest.mark.gpu

torch.cuda.is_available()   # (torch's runtime first, as in the other GPU files)

CASES = ac.cases()
DT = ac.DT
PEM_E_INVALID, PEM_E_STATE = -1, -6
POISON = -7.0
_ORACLE = []


@pytest.fixture(scope="module", autouse=True)
def _bind_oracle(oracle):
    _ORACLE[:] = [oracle]


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


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    return bool(np.all((got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want))))


@functools.lru_cache(maxsize=None)
def _levels(name, smooth, coarse, dt):
    case, sym = CASES[name]
    return ar.hierarchy(case, DT[dt], _ORACLE[0], smooth, int(sym), ac.SEED, ac.MAX_LEVELS, coarse, ac.OMEGA)


@functools.lru_cache(maxsize=None)
def _cycle_ref(name, smooth, coarse, sweeps, coarse_sweeps, dt):
    n = CASES[name][0][0]
    b, _ = ac.rhs(name, n, DT[dt])
    return ar.apply(_levels(name, smooth, coarse, dt), b, _ORACLE[0], sweeps, coarse_sweeps)


@functools.lru_cache(maxsize=None)
def _solve_ref(name, method, smooth, coarse, sweeps, coarse_sweeps, dt, max_iters=ac.MAX_ITERS):
    n = CASES[name][0][0]
    b, x0 = ac.rhs(name, n, DT[dt])
    return ar.solve(_levels(name, smooth, coarse, dt), b, x0, _ORACLE[0], method, sweeps, coarse_sweeps, max_iters, ac.rtol(DT[dt]))


_TILINGS = {}


def _coo_tiling(pkg, ctx, case, dtype):
    n, I, J, V = case
    return pkg.Tiled.from_coo(ctx, n, n, np.asarray(I, np.int32), np.asarray(J, np.int32), np.asarray(V, np.float64), dtype=dtype)


def _tiling(pkg, ctx, name, dt):
    if (name, dt) not in _TILINGS:
        _TILINGS[(name, dt)] = _coo_tiling(pkg, ctx, CASES[name][0], DT[dt])
    return _TILINGS[(name, dt)]


@pytest.fixture(scope="module", autouse=True)
def _drop_tilings():
    yield
    for A in _TILINGS.values():
        A.close()
    _TILINGS.clear()


def _amg(pkg, ctx, name, smooth, coarse, sweeps, coarse_sweeps, dt, **kw):
    return pkg.Amg(_tiling(pkg, ctx, name, dt), smooth=bool(smooth), symmetric=CASES[name][1], seed=ac.SEED, max_levels=ac.MAX_LEVELS,
                   coarse_size=coarse, sweeps=sweeps, coarse_sweeps=coarse_sweeps, omega=ac.OMEGA, **kw)


def _matches(T, M):
    """a tiling against the model's (rows, cols, rp, ci, v)"""
    rows, cols, rp, ci, v = M
    grp, gci, gv = T.export_csr()
    return (T.rows, T.cols) == (rows, cols) and np.array_equal(grp, rp) and np.array_equal(gci, ci) and _same(gv, v)


def _check_levels(M, levels):
    assert M.levels == len(levels)
    for l, L in enumerate(levels):
        A_l, P_l, R_l = M.level(l)
        assert _matches(A_l, L["A"]), l
        if L["P"] is None:
            assert P_l is None and R_l is None
        else:
            assert _matches(P_l, L["P"]) and _matches(R_l, L["R"]), l


def _check_info(M, levels, sweeps, coarse_sweeps):
    info = M.info
    want = ar.info(levels, sweeps, coarse_sweeps)
    assert {k: info[k] for k in want} == want
    assert info["bytes"] > 0 and info["operator_complexity"] == sum(want["nnz"]) / want["nnz"][0]


@pytest.mark.parametrize("name", list(CASES))
def test_hierarchy_and_cycle_match_the_model(pkg, tctx, name):
    """over the whole option grid of the case (one item per case keeps the suite's item count down)"""
    for k, (smooth, coarse, dt) in enumerate(ac.hierarchy_grid()):
        _hierarchy_and_cycle(pkg, tctx, name, smooth, coarse, dt, refreshable=bool(k & 1))


def _hierarchy_and_cycle(pkg, tctx, name, smooth, coarse, dt, refreshable):
    """info and one V-cycle on the case's b for both sweep settings (two applies are identical); every level's A_l, P_l, R_l under
    the first -- the hierarchy does not depend on the sweeps"""
    levels = _levels(name, smooth, coarse, dt)
    n = CASES[name][0][0]
    b, _ = ac.rhs(name, n, DT[dt])
    db = _dev(b)
    for k, (sweeps, coarse_sweeps) in enumerate(ac.SWEEPS):
        M = _amg(pkg, tctx, name, smooth, coarse, sweeps, coarse_sweeps, dt, refreshable=refreshable)
        try:
            _check_info(M, levels, sweeps, coarse_sweeps)
            if k == 0:
                _check_levels(M, levels)
            z = M.apply(db)
            z2 = torch.full_like(db, POISON)
            assert M.apply(db, out=z2) is z2
            want = _cycle_ref(name, smooth, coarse, sweeps, coarse_sweeps, dt)
            assert _same(z.cpu().numpy(), want) and _same(z2.cpu().numpy(), want), (smooth, coarse, sweeps, coarse_sweeps, dt)
        finally:
            M.close()


ROUTE = [("poisson_40", 1, 8, "f64"), ("gen_tridiagonal_200", 1, 8, "f32"), ("spd_grid_40x40_red_black", 0, 40, "f32")]


@pytest.mark.parametrize("name,smooth,coarse,dt", ROUTE, ids=["-".join(map(str, c)) for c in ROUTE])
def test_levels_equal_the_public_calls(pkg, tctx, name, smooth, coarse, dt):
    """the contract's sequence made through the binding: aggregate, prolongator, CPlan + from_cplan, scale, ewise, transpose"""
    A = _tiling(pkg, tctx, name, dt)
    sym = CASES[name][1]
    M = _amg(pkg, tctx, name, smooth, coarse, 1, 4, dt)
    tdt = getattr(torch, np.dtype(DT[dt]).name)
    omega = torch.tensor(ac.OMEGA, dtype=torch.float64).to(tdt).cuda()   # rounded once to the value type
    made = []

    def product(X, Y):
        plan = pkg.CPlan(tctx, X, Y)
        plan.spgemm()
        T = pkg.Tiled.from_cplan(plan)
        plan.close()
        made.append(T)
        return T

    def equal(T, U):
        (a, b, c), (d, e, f) = T.export_csr(), U.export_csr()
        return (T.rows, T.cols) == (U.rows, U.cols) and np.array_equal(a, d) and np.array_equal(b, e) and _same(c, f)

    try:
        cur, l = A, 0
        while True:
            A_l, P_l, R_l = M.level(l)
            assert equal(A_l, cur)
            if l + 1 == ac.MAX_LEVELS or cur.rows <= coarse:
                break
            agg, _, nc, _ = cur.aggregate(seed=ac.SEED, symmetric=sym)
            if nc == cur.rows:
                break
            Pt = pkg.prolongator(tctx, agg, nc, dtype=DT[dt])
            made.append(Pt)
            P = Pt
            if smooth:
                D = cur.select("diag", 0)
                made.append(D)
                w = omega / D.reduce("plus")
                torch.cuda.current_stream().synchronize()
                W = product(cur, Pt).scale(rows=w)
                made.append(W)
                P = pkg.Tiled.ewise(Pt, W, "plus", "union", 1.0, -1.0)
                made.append(P)
            R = P.transpose()
            made.append(R)
            assert equal(P_l, P) and equal(R_l, R)
            cur = product(R, product(cur, P))
            l += 1
        assert M.levels == l + 1 and M.level(l)[1] is None
    finally:
        M.close()
        for T in made:
            T.close()


APPLY = [("poisson_40", 1, 40, 1, 4, "f64"), ("spd_tridiagonal_4097", 0, 8, 2, 1, "f32"), ("spd_dense_17", 1, 40, 1, 4, "f64"),
         ("spd_hubs_1600", 1, 8, 2, 1, "f64")]


@pytest.mark.parametrize("name,smooth,coarse,sweeps,coarse_sweeps,dt", APPLY, ids=["-".join(map(str, c)) for c in APPLY])
def test_apply_launches_and_allocations(pkg, tctx, name, smooth, coarse, sweeps, coarse_sweeps, dt):
    """info.launches is the kernel-statistics call delta of one apply, split into amg_* and mxv kernels as the header states; an
    apply allocates nothing"""
    M = _amg(pkg, tctx, name, smooth, coarse, sweeps, coarse_sweeps, dt)
    n = CASES[name][0][0]
    db = _dev(ac.rhs(name, n, DT[dt])[0])
    z = torch.empty_like(db)
    try:
        M.apply(db, out=z)   # (nothing is built on a first apply; this one only warms the kernels)
        tctx.synchronize()
        before = tctx.memory_stats()
        tctx.set_kernel_profiling(True)
        tctx.reset_kernel_stats()
        try:
            M.apply(db, out=z)
            tctx.synchronize()
            stats = tctx.kernel_stats()
        finally:
            tctx.set_kernel_profiling(False)
        after = tctx.memory_stats()
        assert (after["block_allocs"], after["driver_allocs"], after["in_use_bytes"]) == (
            before["block_allocs"], before["driver_allocs"], before["in_use_bytes"])
        calls = {k: s["calls"] for k, s in stats.items() if s["calls"]}
        L = M.levels
        assert sum(calls.values()) == M.info["launches"] == ar.launches(_levels(name, smooth, coarse, dt), sweeps, coarse_sweeps)
        own = {k: v for k, v in calls.items() if k.startswith("amg_")}
        mxv = sum(v for k, v in calls.items() if k.startswith("mxv_kernel"))
        assert sum(own.values()) + mxv == sum(calls.values())
        want = {"amg_scale": L, "amg_jacobi": (L - 1) * (2 * sweeps - 1) + coarse_sweeps - 1, "amg_residual": L - 1}
        assert own == {k: v for k, v in want.items() if v}
        assert mxv == (L - 1) * (2 * sweeps - 1 + 3) + coarse_sweeps - 1
        assert _same(z.cpu().numpy(), _cycle_ref(name, smooth, coarse, sweeps, coarse_sweeps, dt))
    finally:
        M.close()


def _run(pkg, ctx, M, name, method, dt, check_every=8, max_iters=ac.MAX_ITERS):
    A = _tiling(pkg, ctx, name, dt)
    b, x0 = ac.rhs(name, A.rows, DT[dt])
    K = pkg.Krylov(A, method=method, precond=M, max_iters=max_iters, check_every=check_every, rtol=ac.rtol(DT[dt]))
    assert K.precond == "amg"
    hist = torch.full((max_iters + 1,), POISON, dtype=torch.float64, device="cuda")
    x, info = K.solve(_dev(b), x=_dev(x0), history=hist)
    K.close()
    return x.cpu().numpy(), hist.cpu().numpy(), info


def _check_solve(got, ref, method, check_every, max_iters, V):
    x, hist, info = got
    k = ref["iters"]
    assert (info["iters"], info["status_code"]) == (k, ref["status"]), (info, kr.STATUS[ref["status"]], k)
    assert _same(x, ref["x"])
    assert _same(hist[:k + 1], ref["history"]) and np.all(hist[k + 1:] == POISON)
    for key in ("bb", "rr", "threshold"):
        assert _same(np.float64(info[key]), np.float64(ref[key])), key
    assert info["readbacks"] == kr.readbacks(ref["stop_iter"], check_every)
    assert info["launches"] == ar.solver_launches(method, ref["stop_iter"], check_every, max_iters, V)


# every case x method x dtype under two corners of the option grid (the full grid is covered by the hierarchy and cycle test above;
# a solve adds the hook alone)
SOLVE_OPTS = ((1, 40, 1, 4), (0, 8, 2, 1))


@pytest.mark.parametrize("name", list(CASES))
def test_solve_matches_the_model(pkg, tctx, name):
    for smooth, coarse, sweeps, coarse_sweeps in SOLVE_OPTS:
        for dt in DT:
            M = _amg(pkg, tctx, name, smooth, coarse, sweeps, coarse_sweeps, dt, refreshable=False)
            try:
                for method in ("cg", "bicgstab") if CASES[name][1] else ("bicgstab",):
                    ref = _solve_ref(name, method, smooth, coarse, sweeps, coarse_sweeps, dt)
                    assert ref["status"] == kr.CONVERGED
                    _check_solve(_run(pkg, tctx, M, name, method, dt), ref, method, 8, ac.MAX_ITERS, M.info["launches"])
            finally:
                M.close()


EVERY = [("poisson_40", "cg", 1, 40, 1, 4, "f64"), ("gen_hubs_1600", "bicgstab", 0, 8, 2, 1, "f32"),
         ("spd_tridiagonal_4097", "bicgstab", 1, 8, 1, 4, "f64")]


@pytest.mark.parametrize("name,method,smooth,coarse,sweeps,coarse_sweeps,dt", EVERY, ids=["-".join(map(str, c)) for c in EVERY])
def test_check_every_changes_no_bit(pkg, tctx, name, method, smooth, coarse, sweeps, coarse_sweeps, dt):
    ref = _solve_ref(name, method, smooth, coarse, sweeps, coarse_sweeps, dt)
    M = _amg(pkg, tctx, name, smooth, coarse, sweeps, coarse_sweeps, dt)
    try:
        for ce in (1, 7, ac.MAX_ITERS):
            _check_solve(_run(pkg, tctx, M, name, method, dt, check_every=ce), ref, method, ce, ac.MAX_ITERS, M.info["launches"])
        assert ref["iters"] >= 2
        ref1 = _solve_ref(name, method, smooth, coarse, sweeps, coarse_sweeps, dt, max_iters=1)   # stopped by max_iters
        assert (ref1["status"], ref1["iters"]) == (kr.MAX_ITERS, 1)
        _check_solve(_run(pkg, tctx, M, name, method, dt, max_iters=1), ref1, method, 8, 1, M.info["launches"])
    finally:
        M.close()


@pytest.mark.parametrize("name,method,smooth,dt", [("poisson_40", "cg", 1, "f64"), ("spd_grid_40x40_red_black", "bicgstab", 0, "f32"),
                                                   ("spd_tridiagonal_200", "cg", 1, "f32")])
def test_refresh_equals_a_fresh_create(pkg, tctx, name, method, smooth, dt):
    """new values on A, then refresh: the levels equal a fresh create's and the model's, the next solve equals the model, and from the
    second refresh on nothing is allocated"""
    dtype = DT[dt]
    (n, I, J, V), sym = CASES[name]
    V2 = np.where(I == J, 1.5 * V, 1.25 * V)   # still symmetric, positive and dominant
    A = _coo_tiling(pkg, tctx, (n, I, J, V), dtype)
    o = np.lexsort((J, I))
    dv, dv2 = _dev(np.asarray(V, dtype)[o]), _dev(np.asarray(V2, dtype)[o])
    kw = dict(smooth=bool(smooth), symmetric=sym, coarse_size=8, sweeps=1, coarse_sweeps=4, omega=ac.OMEGA)
    M = pkg.Amg(A, **kw)
    K = pkg.Krylov(A, method=method, precond=M, max_iters=ac.MAX_ITERS, rtol=ac.rtol(dtype))
    levels2 = ar.hierarchy((n, I, J, V2), dtype, _ORACLE[0], smooth, int(sym), 0, 16, 8, ac.OMEGA)
    b, x0 = ac.rhs(name, n, dtype)
    try:
        A.set_values_device(dv2)
        M.refresh()   # (the first refresh builds the refresh maps)
        _check_levels(M, levels2)
        F = pkg.Amg(A, **kw)
        try:
            for l in range(F.levels):
                for T, U in zip(M.level(l), F.level(l)):
                    assert (T is None) == (U is None)
                    if T is not None:
                        (a, b_, c), (d, e, f) = T.export_csr(), U.export_csr()
                        assert np.array_equal(a, d) and np.array_equal(b_, e) and _same(c, f)
            assert {k: v for k, v in F.info.items() if k != "bytes"} == {k: v for k, v in M.info.items() if k != "bytes"}
        finally:
            F.close()
        A.set_values_device(dv)
        M.refresh()
        _check_levels(M, _levels(name, smooth, 8, dt))
        x, info = K.solve(_dev(b), x=_dev(x0))
        ref = _solve_ref(name, method, smooth, 8, 1, 4, dt)
        assert (info["iters"], info["status_code"]) == (ref["iters"], ref["status"]) and _same(x.cpu().numpy(), ref["x"])
        db, dx = _dev(b), _dev(x0)
        tctx.synchronize()
        before = tctx.memory_stats()["block_allocs"]
        A.set_values_device(dv2)
        M.refresh()
        x, info = K.solve(db, x=dx)
        assert tctx.memory_stats()["block_allocs"] == before
        ref2 = ar.solve(levels2, b, x0, _ORACLE[0], method, 1, 4, ac.MAX_ITERS, ac.rtol(dtype))
        assert (info["iters"], info["status_code"]) == (ref2["iters"], ref2["status"]) and _same(x.cpu().numpy(), ref2["x"])
    finally:
        K.close()
        M.close()
        A.close()


def test_not_refreshable(pkg, tctx):
    for smooth in (0, 1):
        # (N first: whatever a first create grows the context's scratch by counts against it, not for it)
        N = _amg(pkg, tctx, "poisson_40", smooth, 8, 1, 4, "f64", refreshable=False)
        M = _amg(pkg, tctx, "poisson_40", smooth, 8, 1, 4, "f64", refreshable=True)
        try:
            assert 0 < N.info["bytes"] < M.info["bytes"]
            assert {k: v for k, v in N.info.items() if k != "bytes"} == {k: v for k, v in M.info.items() if k != "bytes"}
            M.refresh()
            with pytest.raises(pkg.PemError, match="refreshable = 0") as e:
                N.refresh()
            assert e.value.status == PEM_E_STATE
            _check_levels(N, _levels("poisson_40", smooth, 8, "f64"))
        finally:
            M.close()
            N.close()


def test_views_do_not_own(pkg, tctx):
    M = _amg(pkg, tctx, "poisson_40", 1, 40, 1, 4, "f64")
    A0, P0, R0 = M.level(0)
    assert A0._h.value == _tiling(pkg, tctx, "poisson_40", "f64")._h.value   # level 0 is A itself, not a copy
    P0.close()
    P0.close()
    _, P0, _ = M.level(0)
    assert _matches(P0, _levels("poisson_40", 1, 40, "f64")[0]["P"])
    x = torch.ones(P0.cols, dtype=torch.float64, device="cuda")
    assert P0.mxv(x).shape[0] == 1600
    with pytest.raises(pkg.PemError):
        M.level(M.levels)
    M.close()


def test_a_false_symmetric_promise(pkg, tctx):
    """a one-way pattern under symmetric=True: no vertex is left without an aggregate (test_amg_cpu.py says why), so the call
    succeeds and the hierarchy is the model's under the same promise"""
    n, I, J = aggref.grid_one_way(40)
    case = (n, np.concatenate([I, np.arange(n)]), np.concatenate([J, np.arange(n)]), np.concatenate([-np.ones(len(I)), np.full(n, 4.0)]))
    A = _coo_tiling(pkg, tctx, case, np.float64)
    for sym in (True, False):
        M = pkg.Amg(A, smooth=True, symmetric=sym, coarse_size=8)
        try:
            _check_levels(M, ar.hierarchy(case, np.float64, _ORACLE[0], 1, int(sym), 0, 16, 8, ac.OMEGA))
        finally:
            M.close()
    A.close()


def test_refusals(pkg, tctx):
    lib = pkg.lib()
    A = _tiling(pkg, tctx, "spd_dense_33", "f64")
    A32 = _tiling(pkg, tctx, "spd_dense_33", "f32")
    B = _tiling(pkg, tctx, "spd_dense_17", "f64")
    R = pkg.Tiled.from_coo(tctx, 3, 4, [0, 1], [1, 2], [1.0, 2.0])
    n = A.rows
    good = dict(smooth=1, symmetric=1, seed=0, max_levels=16, coarse_size=8, sweeps=1, coarse_sweeps=4, omega=2 / 3, refreshable=1)

    def create(A_=A, ctx=True, opts=True, out=True, **kw):
        o = pkg.AmgOpts(**{**good, **kw})
        h = C.c_void_p(1)
        st = lib.pem_amg_create(tctx._h if ctx else None, A_._h if A_ is not None else None, C.byref(o) if opts else None,
                                C.byref(h) if out else None)
        if st == 0:
            lib.pem_amg_destroy(tctx._h, h)
        else:
            assert not out or not h.value
        return st

    assert create() == 0
    for kw in (dict(ctx=False), dict(A_=None), dict(opts=False), dict(out=False), dict(A_=R), dict(smooth=2), dict(smooth=-1),
               dict(symmetric=2), dict(refreshable=-1), dict(max_levels=0), dict(max_levels=17), dict(coarse_size=0), dict(sweeps=0),
               dict(coarse_sweeps=0), dict(omega=0.0), dict(omega=-0.5), dict(omega=float("inf")), dict(omega=float("nan"))):
        assert create(**kw) == PEM_E_INVALID, kw
        assert b"pem_amg_create" in lib.pem_last_error()
    # a missing diagonal: at level 0, and on the empty tiling (no binding route makes a 0 x 0 tiling: the empty one is n = 40)
    (pn, I, J, V), _ = CASES["poisson_40"]
    keep = ~((I == J) & ((I == 6) | (I == 9)))
    H = _coo_tiling(pkg, tctx, (pn, I[keep], J[keep], V[keep]), np.float64)
    with pytest.raises(pkg.PemError, match=r"pem_amg_create: level 0: row 7 has no stored diagonal entry \(2 such rows\)") as e:
        pkg.Amg(H)
    assert e.value.status == PEM_E_INVALID
    E = pkg.Tiled.from_coo(tctx, 40, 40, [], [], [])
    with pytest.raises(pkg.PemError, match=r"level 0: row 1 has no stored diagonal entry \(40 such rows\)"):
        pkg.Amg(E)
    # a stored zero on the diagonal is legal: an infinite weight, and the solver stops on what is not finite, as the model does
    (dn, I, J, V), _ = CASES["spd_dense_15"]
    zcase = (dn, I, J, np.where((I == J) & (I == 3), 0.0, V))
    Z = _coo_tiling(pkg, tctx, zcase, np.float64)
    MZ = pkg.Amg(Z, symmetric=True)
    for method in ("cg", "bicgstab"):
        x, info = Z.solve(torch.ones(dn, dtype=torch.float64, device="cuda"), method=method, precond=MZ, max_iters=10)
        zref = ar.solve(ar.hierarchy(zcase, np.float64, _ORACLE[0], 1, 1), np.ones(dn), np.zeros(dn), _ORACLE[0], method, max_iters=10)
        assert info["status_code"] == zref["status"] != kr.CONVERGED and info["iters"] == zref["iters"]
        assert info["status"] in ("nonfinite", "breakdown")
    MZ.close()
    # apply
    M = pkg.Amg(A, symmetric=True, coarse_size=8)
    M32 = pkg.Amg(A32, symmetric=True, coarse_size=8)
    other = pkg.Context(0)
    buf = torch.full((3 * n,), POISON, dtype=torch.float64, device="cuda")
    r, z = buf[:n], buf[n:2 * n]
    torch.cuda.current_stream().synchronize()

    def apply(M_, r_, z_, fn=lib.pem_amg_apply, ctx=tctx):
        p = [C.c_void_p(t.data_ptr()) if t is not None else None for t in (r_, z_)]
        return fn(ctx._h if ctx is not None else None, M_._h if M_ is not None else None, *p)

    for args, kw in (((M, r, z), dict(ctx=None)), ((None, r, z), {}), ((M, None, z), {}), ((M, r, None), {}), ((M, r, r), {}),
                     ((M, r, buf[n - 1:2 * n - 1]), {}), ((M, buf[1:n + 1], r), {}), ((M, r, z), dict(ctx=other)),
                     ((M, r, z), dict(fn=lib.pem_amg_apply_f32)), ((M32, r, z), {})):
        assert apply(*args, **kw) == PEM_E_INVALID, (args[1:], kw)
        assert b"pem_amg_apply" in lib.pem_last_error()
    tctx.synchronize()
    assert bool((buf == POISON).all())   # outputs untouched
    assert lib.pem_amg_refresh(other._h, M._h) == PEM_E_INVALID and lib.pem_amg_refresh(tctx._h, None) == PEM_E_INVALID
    # the Krylov hook
    MB = pkg.Amg(B, symmetric=True)

    def kcreate(A_, M_, precond=3, ctx=tctx, fn=lib.pem_krylov_create_amg):
        o = pkg.KrylovOpts(0, precond, 10, 1, 1e-8, 0.0)
        h = C.c_void_p(1)
        st = fn(ctx._h, A_._h, C.byref(o), M_._h if M_ is not None else None, C.byref(h))
        if st == 0:
            lib.pem_krylov_destroy(tctx._h, h)
        else:
            assert not h.value
        return st

    assert kcreate(A, M) == 0
    for args, kw in (((A, MB), {}), ((B, M), {}), ((A, None), {}), ((A, M), dict(precond=2)), ((A, M), dict(precond=0)),
                     ((A, M), dict(ctx=other))):
        assert kcreate(*args, **kw) == PEM_E_INVALID, (args, kw)
        assert b"pem_krylov_create_amg" in lib.pem_last_error()
    assert kcreate(A, None, fn=lib.pem_krylov_create) == PEM_E_INVALID and b"pem_krylov_create:" in lib.pem_last_error()
    with pytest.raises(pkg.PemError):
        pkg.Krylov(A, precond=MB)
    # the Python argument checks
    tb = torch.zeros(n, dtype=torch.float64, device="cuda")
    for bad in (lambda: pkg.Amg(A, max_levels=0), lambda: pkg.Amg(A, max_levels=17), lambda: pkg.Amg(A, coarse_size=0),
                lambda: pkg.Amg(A, sweeps=1.5), lambda: pkg.Amg(A, coarse_sweeps=True), lambda: pkg.Amg(A, omega=0),
                lambda: pkg.Amg(A, omega="x"), lambda: pkg.Amg(A, omega=float("nan")), lambda: pkg.Amg(A, seed=-1), lambda: pkg.Amg(None),
                lambda: M.apply(tb[:-1]), lambda: M.apply(tb.cpu()), lambda: M32.apply(tb), lambda: M.level("0"),
                lambda: pkg.Krylov(A, precond="amg"), lambda: pkg.Krylov(A, precond="ilu"), lambda: A.solve(tb, precond="ssor"),
                lambda: A.solve(tb, precond="ilu")):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(pkg.PemError):
        pkg.Amg(R)
    for h in (M, M32, MB, R, H, E, Z):
        h.close()
    other.close()


@pytest.mark.parametrize("dt", list(DT))
def test_one_shot(pkg, tctx, dt):
    """Tiled.solve with "amg" (its own default Amg, made and closed) and with an Amg instance; torch reads x on the context's stream"""
    name = "poisson_40"
    dtype = DT[dt]
    A = _tiling(pkg, tctx, name, dt)
    b, x0 = ac.rhs(name, A.rows, dtype)
    levels = ar.hierarchy(CASES[name][0], dtype, _ORACLE[0], 1, 0, 0, 16, 40, ac.OMEGA)   # the defaults: symmetric = 0
    x, info = A.solve(_dev(b), method="cg", precond="amg", x=_dev(x0), max_iters=ac.MAX_ITERS, rtol=ac.rtol(dtype), history=True)
    got = (x * 1).cpu().numpy()
    ref = ar.solve(levels, b, x0, _ORACLE[0], "cg", 1, 4, ac.MAX_ITERS, ac.rtol(dtype))
    assert _same(got, ref["x"]) and info["status"] == "converged" and _same(info["history"].cpu().numpy(), ref["history"])
    M = pkg.Amg(A)
    x, info = A.solve(_dev(b), method="bicgstab", precond=M, x=_dev(x0), max_iters=ac.MAX_ITERS, rtol=ac.rtol(dtype))
    ref = ar.solve(levels, b, x0, _ORACLE[0], "bicgstab", 1, 4, ac.MAX_ITERS, ac.rtol(dtype))
    assert _same(x.cpu().numpy(), ref["x"]) and info["iters"] == ref["iters"]
    M.close()
