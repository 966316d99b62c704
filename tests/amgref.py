"""Host model of the aggregation multigrid (include/pem_spgemm.h pem_amg_*), composed from the existing
references: aggref.aggregate for the aggregates, the oracle's product for every plan and every fma chain (as mxvref takes it),
applyref.scale for the row scaling, ewiseref.ewise for the smoothed prolongator, extractref.transpose for R, and krylovref.solve
for the solvers -- its LU slot is given the V-cycle as a callback, so the scalar logic is krylovref's own, line by line.

A matrix is (rows, cols, rp, ci, v): CSR with sorted columns, rp int64, values in the level's dtype.
"""
import numpy as np

import aggref
import applyref
import ewiseref
import extractref
import krylovref as kr
import mxvref

MAX_LEVELS = 16


def check_opts(smooth=1, symmetric=0, seed=0, max_levels=16, coarse_size=40, sweeps=1, coarse_sweeps=4, omega=2 / 3, refreshable=1):
    """the refusals of pem_amg_create's option struct: ValueError"""
    for name, v in (("smooth", smooth), ("symmetric", symmetric), ("refreshable", refreshable)):
        if v not in (0, 1):
            raise ValueError(f"{name} must be 0 or 1")
    if not 0 <= seed < 2 ** 32:
        raise ValueError("seed outside [0, 2^32)")
    if not 1 <= max_levels <= MAX_LEVELS:
        raise ValueError("max_levels outside 1 .. 16")
    for name, v in (("coarse_size", coarse_size), ("sweeps", sweeps), ("coarse_sweeps", coarse_sweeps)):
        if v < 1:
            raise ValueError(f"{name} < 1")
    if not (omega > 0 and np.isfinite(omega)):
        raise ValueError("omega must be positive and finite")


def _coo(M):
    rows, cols, rp, ci, v = M
    return np.repeat(np.arange(rows, dtype=np.int64), np.diff(rp)), np.asarray(ci, np.int64), v


def _csr(rows, cols, I, J, V, dtype):
    """canonical COO (sorted by (row, column)) -> the matrix tuple"""
    rp = np.zeros(rows + 1, np.int64)
    np.cumsum(np.bincount(np.asarray(I, np.int64), minlength=rows), out=rp[1:])
    return rows, cols, rp, np.asarray(J, np.int64), np.asarray(V, dtype)


def product(oracle, A, B, dtype):
    """A B: the plan's C under plus_times, symbolic pattern, one fma chain per entry"""
    Ia, Ja, Va = _coo(A)
    Ib, Jb, Vb = _coo(B)
    a = oracle.Csr(A[0], A[1], Ia, Ja, np.asarray(Va, np.float64))
    b = oracle.Csr(B[0], B[1], Ib, Jb, np.asarray(Vb, np.float64))
    rp, ci, v = oracle.csr_spgemm(a, b, f32=np.dtype(dtype) == np.float32).arrays()
    return A[0], B[1], np.asarray(rp, np.int64), np.asarray(ci, np.int64), np.asarray(v).astype(dtype)


def weights(A, omega, dtype, level=0):
    """w_i = (VT)omega / d_i; a row without a stored diagonal entry: ValueError in the wording of the library's refusal"""
    rows, _, rp, ci, v = A
    I, J, V = _coo(A)
    on = I == J
    has = np.zeros(rows, bool)
    has[I[on]] = True
    if not has.all():
        miss = np.flatnonzero(~has)
        raise ValueError(f"level {level}: row {miss[0] + 1} has no stored diagonal entry ({len(miss)} such rows)")
    d = np.zeros(rows, dtype)
    d[I[on]] = V[on]
    with np.errstate(all="ignore"):
        return (np.dtype(dtype).type(omega) / d).astype(dtype)


def hierarchy(case, dtype, oracle, smooth=1, symmetric=0, seed=0, max_levels=16, coarse_size=40, omega=2 / 3):
    """the levels of pem_amg_create on the case (n, I, J, V): a list of dicts A, w, rounds and, above the coarsest, P, R"""
    dtype = np.dtype(dtype).type
    check_opts(smooth, symmetric, seed, max_levels, coarse_size, 1, 1, omega)
    n, I, J, V = case
    I, J, V = ewiseref.canonical(I, J, np.asarray(V, dtype), n)
    A = _csr(n, n, I, J, V, dtype)
    levels = []
    while True:
        l = len(levels)
        n = A[0]
        L = dict(A=A, w=weights(A, omega, dtype, l) if n else np.zeros(0, dtype), rounds=0, P=None, R=None)
        levels.append(L)
        if n == 0 or l + 1 == max_levels or n <= coarse_size:
            break
        Ia, Ja, _ = _coo(A)
        agg, _, nc, L["rounds"] = aggref.aggregate(n, Ia, Ja, seed=seed, symmetric=bool(symmetric))
        if nc == n:
            break
        if np.any(np.asarray(agg) < 0):
            raise ValueError(f"level {l}: {int(np.sum(np.asarray(agg) < 0))} vertices have no aggregate; pass symmetric = 0")
        Pt = _csr(n, nc, np.arange(n), np.asarray(agg, np.int64), np.ones(n, dtype), dtype)
        if smooth:
            T = product(oracle, A, Pt, dtype)
            It, Jt, Vt = _coo(T)
            W = applyref.scale(It, Jt, Vt, r=L["w"], op="times", dtype=dtype)
            Ip, Jp, Vp = ewiseref.ewise(nc, _coo(Pt), (It, Jt, W), "plus", "union", 1.0, -1.0)
            P = _csr(n, nc, Ip, Jp, Vp, dtype)
        else:
            P = Pt
        _, _, Ir, Jr, Vr = extractref.transpose(n, nc, *_coo(P))
        R = _csr(nc, n, Ir, Jr, Vr, dtype)
        L["P"], L["R"] = P, R
        A = product(oracle, R, product(oracle, A, P, dtype), dtype)
    return levels


def launches(levels, sweeps, coarse_sweeps):
    """pem_amg_info::launches: the kernel launches of one apply"""
    out = 0
    for l, L in enumerate(levels):
        if L["A"][0]:
            out += 2 * coarse_sweeps - 1 if l + 1 == len(levels) else 4 * sweeps + 3
    return out


def info(levels, sweeps, coarse_sweeps):
    """what Amg.info holds, bytes apart"""
    return dict(levels=len(levels), rows=[L["A"][0] for L in levels], nnz=[len(L["A"][3]) for L in levels],
                p_nnz=[len(L["P"][3]) if L["P"] is not None else 0 for L in levels], aggregate_rounds=[L["rounds"] for L in levels],
                launches=launches(levels, sweeps, coarse_sweeps))


def _mxv(oracle, M, x, dtype, y0=None):
    rows, cols, rp, ci, v = M
    return mxvref.mxv(rows, cols, rp, ci, v, x, "plus_times", dtype, y0=y0, oracle=oracle)


def apply(levels, r, oracle, sweeps=1, coarse_sweeps=4):
    """z = one V-cycle from z = 0: every product and sum rounded once in the dtype, every A x the fma chain"""
    dtype = levels[0]["w"].dtype.type
    if levels[0]["A"][0] == 0:
        return np.zeros(0, dtype)

    def jacobi(L, b, x, count):
        for _ in range(count):
            q = _mxv(oracle, L["A"], x, dtype)
            x = x + L["w"] * (b - q)
        return x

    def cycle(l, b):
        L = levels[l]
        x = L["w"] * b
        if l + 1 == len(levels):
            return jacobi(L, b, x, coarse_sweeps - 1)
        x = jacobi(L, b, x, sweeps - 1)
        res = b - _mxv(oracle, L["A"], x, dtype)
        xc = cycle(l + 1, _mxv(oracle, L["R"], res, dtype))
        x = _mxv(oracle, L["P"], xc, dtype, y0=x)
        return jacobi(L, b, x, sweeps)

    with np.errstate(all="ignore"):
        return cycle(0, np.asarray(r, dtype))


class _Callback:
    """stands where krylovref keeps trsvref: the lower solve is the callback, the upper one the identity"""

    def __init__(self, cb):
        self.cb = cb

    def trsv(self, n, rp, ci, v, r, uplo, unit_diag, dtype):
        return self.cb(r) if uplo == "lower" else r


def solve(levels, b, x0, oracle, method="cg", sweeps=1, coarse_sweeps=4, max_iters=200, rtol=1e-8, atol=0.0, precond=None):
    """krylovref.solve on level 0's matrix with z = precond(r) where LU has its two solves; precond defaults to the V-cycle"""
    n, _, rp, ci, v = levels[0]["A"]
    dtype = levels[0]["w"].dtype.type
    cb = precond or (lambda r: apply(levels, r, oracle, sweeps, coarse_sweeps))
    saved = kr.trsvref
    kr.trsvref = _Callback(cb)
    try:
        return kr.solve(n, rp, ci, v, b, x0, method, "lu", factor=(None, None, None), max_iters=max_iters, rtol=rtol, atol=atol, dtype=dtype,
                        oracle=oracle)
    finally:
        kr.trsvref = saved


def solver_launches(method, stop_iter, check_every, max_iters, V):
    """res->launches with the trsv term replaced by V"""
    return kr.launches(method, "lu", stop_iter, check_every, max_iters, V)
