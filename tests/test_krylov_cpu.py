"""CPU: the numpy statement of the Krylov solvers (krylovref.py) is a correct CG / BiCGStab, its cases converge, every status is
reached by construction, and the ctypes view of the pem_krylov_* ABI matches the header."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import ilu0ref as ir
import krylovcases as kc
import krylovref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = kc.cases()
COMBOS = [(name, m, pc) for name, (_, spd) in CASES.items() for m in (("cg", "bicgstab") if spd else ("bicgstab",))
          for pc in ("none", "diag", "lu")]


@functools.lru_cache(maxsize=None)
def _system(name):
    n, rp, ci, v = kc.csr(CASES[name][0], np.float64)
    b, x0 = kc.rhs(name, n)
    I = np.repeat(np.arange(n), np.diff(rp))
    minv = 1.0 / v[I == ci]
    f, _ = ir.ilu0(n, rp, ci, v, np.float64)
    return n, rp, ci, v, b, x0, minv, f


def _small(rows, b, oracle, method, **kw):
    """the reference on a small dense matrix, zero guess"""
    A = sp.csr_matrix(np.array(rows, float))
    A.sort_indices()
    n = A.shape[0]
    return kr.solve(n, A.indptr, A.indices, A.data, np.array(b, float), np.zeros(n), method, oracle=oracle, **kw)


def test_spd_cases_are_symmetric_positive_definite():
    for name, (case, spd) in CASES.items():
        if spd and case[0] <= 200:
            n, I, J, V = case
            M = sp.coo_matrix((V, (I, J)), shape=(n, n)).toarray()
            assert np.array_equal(M, M.T), name
            assert np.linalg.eigvalsh(M).min() > 0, name


@pytest.mark.parametrize("name,method,precond", COMBOS, ids=["-".join(c) for c in COMBOS])
def test_reference_converges_to_a_true_solution(oracle, name, method, precond):
    """CONVERGED within MAX_ITERS at RTOL, and the true residual ||b - A x||_2 (scipy, fp64) is at most 2 sqrt(threshold): the gap
    between the recurrence residual and the true one is of order eps ||A|| ||x|| iters, about 1e-14 here, six orders below the
    threshold, so the factor 2 fails only on a wrong algorithm"""
    n, rp, ci, v, b, x0, minv, f = _system(name)
    r = kr.solve(n, rp, ci, v, b, x0, method, precond, minv=minv, factor=(rp, ci, f), max_iters=kc.MAX_ITERS, rtol=kc.RTOL, oracle=oracle)
    assert r["status"] == kr.CONVERGED and 0 < r["iters"] <= kc.MAX_ITERS
    assert len(r["history"]) == r["iters"] + 1 and r["history"][-1] == r["rr"] <= r["threshold"]
    assert r["threshold"] == (kc.RTOL * kc.RTOL) * r["bb"]
    A = sp.csr_matrix((v, ci, rp), shape=(n, n))
    true = np.linalg.norm(b - A @ r["x"])
    print(f"{name} {method} {precond}: iters {r['iters']} true residual {true:.3e} sqrt(threshold) {np.sqrt(r['threshold']):.3e}")
    assert true <= 2 * np.sqrt(r["threshold"])


def test_dot_is_a_dot_at_the_partition_edges():
    rng = np.random.default_rng(5)
    for n in (1, 255, 257, 4095, 4096, 4097, 3 * 4096 + 5):
        for dt in (np.float64, np.float32):
            u, v = rng.standard_normal(n).astype(dt), rng.standard_normal(n).astype(dt)
            want = float(np.dot(u.astype(np.float64), v.astype(np.float64)))
            assert abs(kr.dot(u, v) - want) <= 1e-12 * max(1.0, float(np.abs(u.astype(np.float64) * v).sum())), (n, dt)
    assert kr.grid(1) == 1 and kr.grid(4096) == 1 and kr.grid(4097) == 2 and kr.grid(4096 * 1024 + 1) == 1024
    assert np.isnan(kr.dot(np.array([1.0, np.nan]), np.array([1.0, 1.0])))


def test_every_status_is_reached(oracle):
    # CG on an indefinite symmetric matrix: p^T A p <= 0 at the first step
    r = _small([[1, 0], [0, -1]], [1, 2], oracle, "cg")
    assert (r["status"], r["iters"], r["reason"], r["stop_iter"]) == (kr.BREAKDOWN, 0, "pq", 1)
    assert np.array_equal(r["x"], np.zeros(2)) and len(r["history"]) == 1
    # b = 0: converged before the first iteration
    for m in ("cg", "bicgstab"):
        r = _small([[2, 1], [1, 3]], [0, 0], oracle, m)
        assert (r["status"], r["iters"], r["stop_iter"]) == (kr.CONVERGED, 0, 0) and len(r["history"]) == 1
    # max_iters = 3 on a case that needs more; max_iters = 0
    n, rp, ci, v, b, x0, minv, f = _system("spd_tridiagonal_200")
    for m in ("cg", "bicgstab"):
        r = kr.solve(n, rp, ci, v, b, x0, m, max_iters=3, rtol=kc.RTOL, oracle=oracle)
        assert (r["status"], r["iters"], r["stop_iter"]) == (kr.MAX_ITERS, 3, 3) and len(r["history"]) == 4
        r = kr.solve(n, rp, ci, v, b, x0, m, max_iters=0, rtol=kc.RTOL, oracle=oracle)
        assert (r["status"], r["iters"]) == (kr.MAX_ITERS, 0) and np.array_equal(r["x"], x0)
    # a NaN in b
    for m in ("cg", "bicgstab"):
        r = _small([[2, 1], [1, 3]], [np.nan, 1], oracle, m)
        assert (r["status"], r["iters"]) == (kr.NONFINITE, 0) and np.isnan(r["rr"])
    # BiCGStab on the 2 x 2 rotation by a right angle: rhat = r = b is orthogonal to v = A r: rv = 0
    r = _small([[0, -1], [1, 0]], [1, 0], oracle, "bicgstab")
    assert (r["status"], r["iters"], r["reason"], r["stop_iter"]) == (kr.BREAKDOWN, 0, "rv", 1)
    # rho' = 0 needs three dimensions (on a 2 x 2 system rv = 0, omega = 0 or convergence comes first): here every step is exact in
    # fp32 and fp64 -- v = (-1, -1, 1), alpha = -1, s = (-1, 0, 1), t = (0, 0, 1), omega = 1, r = (-1, 0, 0), orthogonal to rhat = b
    r = _small(RHO_MATRIX, RHO_B, oracle, "bicgstab")
    assert (r["status"], r["iters"], r["reason"], r["stop_iter"]) == (kr.BREAKDOWN, 1, "rho", 1)
    assert np.array_equal(r["x"], [-1.0, -1.0, 1.0]) and np.array_equal(r["history"], [1.0, 1.0])


RHO_MATRIX = [[-1, -1, -1], [-1, -1, -1], [-1, 1, 0]]
RHO_B = [0, 1, 0]


def test_launch_formula():
    assert kr.readbacks(0, 8) == 1 and kr.readbacks(8, 8) == 1 and kr.readbacks(9, 8) == 2
    assert kr.launches("cg", "none", 0, 8, 0) == 3
    assert kr.launches("cg", "none", 9, 8, 200) == 3 + 16 * 4
    assert kr.launches("cg", "lu", 3, 7, 5, trsv_launches=4) == 8 + 5 * 9
    assert kr.launches("bicgstab", "lu", 1, 1, 10, trsv_launches=2) == 3 + 11


def _declared_block():
    text = open(os.path.join(ROOT, "include", "pem_spgemm.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_ctypes_signatures_match_the_header(pkg):
    text = _declared_block()
    assert re.search(r"enum \{ PEM_KRYLOV_CG = 0, PEM_KRYLOV_BICGSTAB = 1 \}", text)
    assert re.search(r"enum \{ PEM_PRECOND_NONE = 0, PEM_PRECOND_DIAG = 1, PEM_PRECOND_LU = 2 \}", text)
    assert re.search(r"PEM_KRYLOV_CONVERGED = 0, PEM_KRYLOV_MAX_ITERS = 1, PEM_KRYLOV_BREAKDOWN = 2, PEM_KRYLOV_NONFINITE = 3", text)
    assert pkg.KRYLOV_METHODS == ("cg", "bicgstab") and pkg.KRYLOV_PRECONDS == ("none", "diag", "lu")
    assert pkg.KRYLOV_STATUS == kr.STATUS
    m = re.search(r"typedef struct \{([^}]*)\} pem_krylov_opts;", text)
    names = re.findall(r"(\w+)\s*[,;]", m.group(1))
    assert names == [f for f, _ in pkg.KrylovOpts._fields_] and C.sizeof(pkg.KrylovOpts) == 40
    m = re.search(r"typedef struct \{([^}]*)\} pem_krylov_result;", text)
    names = re.findall(r"(\w+)\s*[,;]", m.group(1))
    assert names == [f for f, _ in pkg.KrylovResult._fields_] and C.sizeof(pkg.KrylovResult) == 56
    assert pkg.KrylovResult.status.offset == 8 and pkg.KrylovResult.bb.offset == 16
    lib = pkg.lib()
    for sym, nargs in (("pem_krylov_create", 5), ("pem_krylov_solve", 7), ("pem_krylov_solve_f32", 7), ("pem_krylov_destroy", 2),
                       ("pem_test_krylov_dot", 6)):
        fn = getattr(lib, sym)
        assert len(fn.argtypes) == nargs and fn.restype is C.c_int, sym
        hdr = "pem_test.h" if sym.startswith("pem_test") else "pem_spgemm.h"
        decl = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", hdr)).read(), flags=re.S)
        args = re.search(r"pem_status " + sym + r"\(([^;]*)\);", decl).group(1)
        assert args.count(",") + 1 == nargs, sym


def test_null_arguments_are_refused_without_a_device(pkg):
    lib = pkg.lib()
    out = C.c_void_p(1)
    opts = pkg.KrylovOpts(0, 0, 10, 1, 1e-8, 0.0)
    assert lib.pem_krylov_create(None, None, C.byref(opts), None, C.byref(out)) == -1 and not out.value
    assert b"pem_krylov_create" in lib.pem_last_error()
    res = pkg.KrylovResult()
    assert lib.pem_krylov_solve(None, None, None, None, None, None, C.byref(res)) == -1
    assert lib.pem_krylov_solve_f32(None, None, None, None, None, None, C.byref(res)) == -1
    d = C.c_double()
    assert lib.pem_test_krylov_dot(None, 0, 8, None, None, C.byref(d)) == -1
    assert lib.pem_krylov_destroy(None, None) == 0
