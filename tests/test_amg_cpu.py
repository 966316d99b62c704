"""CPU: the host model of the aggregation multigrid (amgref.py) is a correct preconditioner -- its V-cycle is a symmetric operator,
every case of the grid converges to a true solution, the iteration counts on the Poisson problem stay under the caps -- and its
stop rules, refusals and level sizes are what the contract states.  These tests pin the reference the GPU tests compare with."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import aggref
import amgcases as ac
import amgref as ar
import krylovref as kr

CASES = ac.cases()
_ORACLE = []


@pytest.fixture(scope="module", autouse=True)
def _bind_oracle(oracle):
    _ORACLE[:] = [oracle]


@functools.lru_cache(maxsize=None)
def _levels(name, smooth, coarse, dt, max_levels=ac.MAX_LEVELS):
    case, sym = CASES[name]
    return ar.hierarchy(case, ac.DT[dt], _ORACLE[0], smooth, int(sym), ac.SEED, max_levels, coarse, ac.OMEGA)


def _rows(levels):
    return [L["A"][0] for L in levels]


# the level sizes the model gives with seed 0 (symmetric = 1 on these cases), recorded
ROWS = {("poisson_40", 0, 40): [1600, 233, 28], ("poisson_40", 1, 40): [1600, 233, 19], ("poisson_40", 0, 8): [1600, 233, 28, 4],
        ("poisson_40", 1, 8): [1600, 233, 19, 1], ("spd_tridiagonal_4097", 1, 40): [4097, 1124, 307, 81, 22],
        ("spd_tridiagonal_4097", 1, 8): [4097, 1124, 307, 81, 22, 6], ("spd_dense_17", 1, 40): [17], ("spd_dense_33", 1, 8): [33, 1],
        ("diag_50", 1, 8): [50], ("spd_hubs_1600", 0, 8): [1600, 1500], ("spd_dense_1", 1, 8): [1]}


@pytest.mark.parametrize("key", list(ROWS), ids=["-".join(map(str, k)) for k in ROWS])
def test_level_sizes(key):
    name, smooth, coarse = key
    for dt in ac.DT:
        levels = _levels(name, smooth, coarse, dt)
        assert _rows(levels) == ROWS[key]
        for L, N in zip(levels, levels[1:]):
            n, nc = L["A"][0], N["A"][0]
            assert L["P"][:2] == (n, nc) and L["R"][:2] == (nc, n) and N["A"][:2] == (nc, nc)
            assert len(L["P"][3]) >= n and L["rounds"] >= 1
        assert levels[-1]["P"] is None and levels[-1]["R"] is None


def test_stop_rules():
    case = CASES["poisson_40"][0]
    o = _ORACLE[0]
    assert _rows(ar.hierarchy(case, np.float64, o, 1, 1, 0, 1, 40)) == [1600]           # max_levels
    assert _rows(ar.hierarchy(case, np.float64, o, 1, 1, 0, 2, 40)) == [1600, 233]
    assert _rows(ar.hierarchy(case, np.float64, o, 1, 1, 0, 16, 233)) == [1600, 233]    # n_l <= coarse_size
    assert _rows(ar.hierarchy(case, np.float64, o, 1, 1, 0, 16, 232)) == [1600, 233, 19]
    stalled = ar.hierarchy(CASES["diag_50"][0], np.float64, o, 1, 1, 0, 16, 8)          # naggregates == n_l
    assert _rows(stalled) == [50] and stalled[0]["rounds"] == 1
    hubs = _levels("spd_hubs_1600", 1, 8, "f64")
    assert _rows(hubs) == [1600, 1500] and hubs[1]["rounds"] == 1


def test_refusals():
    good = dict(smooth=1, symmetric=0, seed=0, max_levels=16, coarse_size=40, sweeps=1, coarse_sweeps=4, omega=2 / 3, refreshable=1)
    ar.check_opts(**good)
    for bad in (dict(smooth=2), dict(symmetric=-1), dict(refreshable=2), dict(seed=2 ** 32), dict(max_levels=0), dict(max_levels=17),
                dict(coarse_size=0), dict(sweeps=0), dict(coarse_sweeps=0), dict(omega=0.0), dict(omega=-1.0), dict(omega=float("inf")),
                dict(omega=float("nan"))):
        with pytest.raises(ValueError):
            ar.check_opts(**{**good, **bad})
    # a row without a stored diagonal entry, at level 0: the level, the first row (1-based) and the count
    n, I, J, V = CASES["poisson_40"][0]
    keep = ~((I == J) & ((I == 6) | (I == 9)))
    with pytest.raises(ValueError, match=r"level 0: row 7 has no stored diagonal entry \(2 such rows\)"):
        ar.hierarchy((n, I[keep], J[keep], V[keep]), np.float64, _ORACLE[0], 1, 1)
    # a one-way pattern under a symmetric = 1 promise.  The refusal of a vertex without an aggregate is in the model and in the
    # library, but no pattern reaches it: a vertex turns out only when it sees a root within two hops of its own rows, the middle
    # vertex of such a path sees the root and is placed by pass 1, so pass 2 places the vertex (6000 random one-way patterns and
    # this grid leave no -1).  What the false promise changes is the aggregation, and with it the hierarchy
    n, I, J = aggref.grid_one_way(40)
    case = (n, np.concatenate([I, np.arange(n)]), np.concatenate([J, np.arange(n)]), np.concatenate([-np.ones(len(I)), np.full(n, 4.0)]))
    assert _rows(ar.hierarchy(case, np.float64, _ORACLE[0], 1, 1)) != _rows(ar.hierarchy(case, np.float64, _ORACLE[0], 1, 0))
    # a stored zero on the diagonal is legal: an infinite weight
    n, I, J, V = CASES["spd_dense_15"][0]
    V = np.where((I == J) & (I == 3), 0.0, V)
    assert np.isinf(ar.hierarchy((n, I, J, V), np.float64, _ORACLE[0], 1, 1)[0]["w"][3])


@pytest.mark.parametrize("smooth,sweeps,coarse_sweeps", [(s, sw, cs) for s in ac.SMOOTH for sw, cs in ac.SWEEPS])
def test_the_cycle_is_a_symmetric_operator(smooth, sweeps, coarse_sweeps):
    """|u^T M v - v^T M u| <= 1e-10 ||u|| ||M v||: in exact arithmetic the cycle with equal pre- and post-smoothing is symmetric for
    a symmetric A; in fp64 each of its O(levels * sweeps) vector operations adds a relative error of order eps = 2.2e-16 times the
    condition of the smoothing steps, orders below 1e-10, while a cycle that is not symmetric (unequal sweeps, R != P^T) misses by a
    relative 1e-2 or more"""
    levels = _levels("poisson_40", smooth, 40, "f64")
    rng = np.random.default_rng(5)
    u, v = rng.standard_normal(1600), rng.standard_normal(1600)
    Mu, Mv = (ar.apply(levels, t, _ORACLE[0], sweeps, coarse_sweeps) for t in (u, v))
    assert abs(u @ Mv - v @ Mu) <= 1e-10 * np.linalg.norm(u) * np.linalg.norm(Mv)
    assert u @ Mu > 0 and v @ Mv > 0


@pytest.mark.parametrize("name", list(CASES))
def test_every_case_converges_to_a_true_solution(name):
    """every method and every option of the grid on the case (one item per case keeps the suite's item count down)"""
    for method in ("cg", "bicgstab") if CASES[name][1] else ("bicgstab",):
        for opt in ac.option_grid():
            _converges(name, method, *opt)


def _converges(name, method, smooth, coarse, sweeps, coarse_sweeps, dt):
    """CONVERGED within MAX_ITERS, and the true residual ||b - A x||_2 (scipy, fp64) is at most 2 sqrt(threshold): the recurrence
    residual and the true one differ by rounding alone, about eps ||A|| ||x|| sqrt(iters) -- 1e-14 in fp64 against 1e-8 ||b||; in
    fp32 (eps = 6e-8, ||A|| < 10, at most 40 iterations, ||x|| <= ||b|| on the dominant cases) 4e-6 ||b|| against 1e-4 ||b|| -- so
    the factor 2 fails only on a wrong algorithm"""
    dtype = ac.DT[dt]
    levels = _levels(name, smooth, coarse, dt)
    n, _, rp, ci, v = levels[0]["A"]
    b, x0 = ac.rhs(name, n, dtype)
    r = ar.solve(levels, b, x0, _ORACLE[0], method, sweeps, coarse_sweeps, ac.MAX_ITERS, ac.rtol(dtype))
    what = (method, smooth, coarse, sweeps, coarse_sweeps, dt)
    assert r["status"] == kr.CONVERGED and 0 < r["iters"] <= ac.MAX_ITERS, what
    assert len(r["history"]) == r["iters"] + 1 and r["history"][-1] == r["rr"] <= r["threshold"], what
    A = sp.csr_matrix((v.astype(np.float64), ci, rp), shape=(n, n))
    true = np.linalg.norm(b.astype(np.float64) - A @ r["x"].astype(np.float64))
    assert true <= 2 * np.sqrt(r["threshold"]), what


def test_iteration_caps_on_the_poisson_problem():
    """defaults, a zero guess: smoothed aggregation takes at most a third of Jacobi-CG's iterations, plain aggregation at most half"""
    name = "poisson_40"
    n, rp, ci, v = ac.csr(CASES[name][0])
    b, _ = ac.rhs(name, n)
    x0 = np.zeros(n)
    I = np.repeat(np.arange(n), np.diff(rp))
    jacobi = kr.solve(n, rp, ci, v, b, x0, "cg", "diag", minv=1.0 / v[I == ci], max_iters=1000, rtol=ac.RTOL, oracle=_ORACLE[0])
    assert jacobi["status"] == kr.CONVERGED
    iters = {}
    for smooth in (1, 0):
        r = ar.solve(_levels(name, smooth, 40, "f64"), b, x0, _ORACLE[0], "cg", 1, 4, 1000, ac.RTOL)
        assert r["status"] == kr.CONVERGED
        iters[smooth] = r["iters"]
    print("jacobi", jacobi["iters"], "smoothed", iters[1], "plain", iters[0])
    assert 3 * iters[1] <= jacobi["iters"]
    assert 2 * iters[0] <= jacobi["iters"]


def test_the_callback_is_krylovref_itself():
    """solve() with the identity as its callback is krylovref's unpreconditioned solve, bit for bit; krylovref is left as it was"""
    name = "spd_tridiagonal_200"
    levels = _levels(name, 1, 40, "f64")
    n, _, rp, ci, v = levels[0]["A"]
    b, x0 = ac.rhs(name, n)
    saved = kr.trsvref
    for method in ("cg", "bicgstab"):
        got = ar.solve(levels, b, x0, _ORACLE[0], method, max_iters=ac.MAX_ITERS, precond=lambda r: r)
        want = kr.solve(n, rp, ci, v, b, x0, method, "none", max_iters=ac.MAX_ITERS, oracle=_ORACLE[0])
        assert got["iters"] == want["iters"] and np.array_equal(got["x"], want["x"]) and np.array_equal(got["history"], want["history"])
    assert kr.trsvref is saved
    assert ar.solver_launches("cg", 9, 8, 200, 11) == (4 + 11) + 16 * (5 + 11)
    assert ar.solver_launches("bicgstab", 9, 8, 200, 11) == 3 + 16 * (7 + 2 * 11)
    assert ar.launches(levels, 1, 4) == 2 * (4 * 1 + 3) + (2 * 4 - 1) and ar.launches(levels, 2, 1) == 2 * (4 * 2 + 3) + 1
