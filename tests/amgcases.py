"""The systems and the option grid of the multigrid tests (test_amg_cpu.py, test_gpu_amg.py, test_gpu_amg_cli.py).

Cases: the 5-point Laplacian on 40 x 40 (poisson_40: diagonal 4, off-diagonal -1, n = 1600), a diagonal matrix that never coarsens
(diag_50), all eight spd_* systems of krylovcases (n = 1, 15, 17, 33, 200, 1600, 1600, 4097) for CG and BiCGStab, and three of its
non-symmetric gen_* systems for BiCGStab.  A case is (n, I, J, V) in float64 with the diagonal stored; the symmetric ones are
aggregated with symmetric=True, the gen_* ones with symmetric=False.  b and the guess come from krylovcases.rhs.

Options: smooth 0 / 1 x coarse_size 8 / 40 x (sweeps, coarse_sweeps) in {(1, 4), (2, 1)} x fp64 / fp32; seed 0, omega 2/3,
max_levels 16 throughout.  What the grid reaches: one level (spd_dense_17 at coarse_size 40), two levels with a 1 x 1 coarse matrix
(spd_dense_33 at 8), stalled coarsening (diag_50, spd_hubs_1600), five and six levels (spd_tridiagonal_4097), three on poisson_40.
"""
import numpy as np

import krylovcases as kc
from krylovcases import MAX_ITERS, RTOL, RTOL32, csr, rhs   # noqa: F401  (for the tests)

DT = {"f64": np.float64, "f32": np.float32}
OMEGA = 2 / 3
SEED = 0
MAX_LEVELS = 16
GEN = ("gen_tridiagonal_200", "gen_dense_33", "gen_hubs_1600")
SMOOTH = (0, 1)
COARSE = (8, 40)
SWEEPS = ((1, 4), (2, 1))


def poisson(k):
    """the 5-point Laplacian on a k x k grid, row-major vertices"""
    idx = np.arange(k * k).reshape(k, k)
    I = [idx.ravel()]
    J = [idx.ravel()]
    V = [np.full(k * k, 4.0)]
    for a, b in ((idx[:, :-1], idx[:, 1:]), (idx[:-1, :], idx[1:, :])):
        for s, t in ((a, b), (b, a)):
            I.append(s.ravel())
            J.append(t.ravel())
            V.append(np.full(s.size, -1.0))
    return k * k, np.concatenate(I), np.concatenate(J), np.concatenate(V)


def diagonal(n):
    return n, np.arange(n), np.arange(n), 1.0 + np.arange(n) % 7


def cases():
    """name -> (case, symmetric: the pattern is symmetric and the matrix positive definite)"""
    out = {"poisson_40": (poisson(40), True), "diag_50": (diagonal(50), True)}
    for name, (case, spd) in kc.cases().items():
        if spd or name in GEN:
            out[name] = (case, spd)
    return out


def rtol(dtype):
    return RTOL if np.dtype(dtype) == np.float64 else RTOL32


def hierarchy_grid():
    """(smooth, coarse_size, dt): what a hierarchy depends on"""
    return [(s, c, dt) for s in SMOOTH for c in COARSE for dt in DT]


def option_grid():
    """(smooth, coarse_size, sweeps, coarse_sweeps, dt)"""
    return [(s, c, sw, cs, dt) for s in SMOOTH for c in COARSE for sw, cs in SWEEPS for dt in DT]
