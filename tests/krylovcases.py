"""The systems of the Krylov tests (test_krylov_cpu.py, test_gpu_krylov.py).

SPD cases: B + B^T on the off-diagonal patterns of ilu0cases with trsvcases' dominant diagonal made positive (symmetric, strictly
diagonally dominant, positive diagonal: positive definite), for CG and BiCGStab.  Non-symmetric cases: the ilu0cases as they are,
for BiCGStab.  The sizes hit the vector kernels' edges: fewer elements than a wave, than a workgroup, one chunk and one element
more than a chunk (4097), and the tile edges of mxv and trsv.  A case is (n, I, J, V) in float64 with the diagonal stored; b and
the guess x0 come from rhs().  Every case converges in the reference within MAX_ITERS at RTOL (fp64; test_krylov_cpu.py checks
it); the fp32 runs stop at RTOL32, above what fp32 residuals can reach."""
import numpy as np

import ilu0cases as ic
from trsvcases import DTYPES, csr   # noqa: F401  (for the tests)

MAX_ITERS = 200
RTOL = 1e-8
RTOL32 = 1e-4
NAMES = ("dense_1", "dense_15", "dense_17", "dense_33", "tridiagonal_200", "grid_40x40_red_black", "hubs_1600", "tridiagonal_4097")


def _base(name):
    if name == "tridiagonal_4097":   # (not an ilu0case; with its diagonal's random signs the plain BiCGStab needs > 200 iterations)
        n, I, J, V = ic.band(4097, 1, 108)
        return n, I, J, np.where(I == J, np.abs(V), V)
    return ic.cases()[name]


def spd(case, seed):
    """B + B^T off the diagonal, a positive dominant diagonal"""
    n, I, J, V = case
    off = I != J
    key = np.concatenate([I[off] * n + J[off], J[off] * n + I[off]])
    val = np.concatenate([V[off], V[off]])
    uk, inv = np.unique(key, return_inverse=True)
    B = np.zeros(len(uk))
    np.add.at(B, inv, val)
    si, sj = uk // n, uk % n
    s = np.zeros(n)
    np.add.at(s, si, np.abs(B))
    d = s + 1.0 + np.random.default_rng(seed).random(n)
    return n, np.concatenate([si, np.arange(n)]), np.concatenate([sj, np.arange(n)]), np.concatenate([B, d])


def cases():
    """name -> (case, is_spd)"""
    out = {}
    for k, name in enumerate(NAMES):
        base = _base(name)
        out["spd_" + name] = (spd(base, 200 + k), True)
        out["gen_" + name] = (base, False)
    return out


def rhs(name, n, dtype=np.float64):
    """(b, x0) of a case: standard normal b, a small random guess"""
    rng = np.random.default_rng(abs(hash_name(name)) % (2 ** 31))
    b = rng.standard_normal(n)
    x0 = 0.1 * rng.standard_normal(n)
    return np.asarray(b, dtype), np.asarray(x0, dtype)


def hash_name(name):
    h = 0
    for ch in name:
        h = (h * 131 + ord(ch)) % (2 ** 31 - 1)
    return h
