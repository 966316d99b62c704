"""GPU: `pemspgemm A.mtx 0 --dup OP --out C.mtx` builds its Matrix-Market operands with pem_tiled_build, folding repeated positions
under OP -- a general file with duplicates and a symmetric file that lists both triangles (whose expansion repeats every
off-diagonal position) -- against scipy's duplicate sum; without --dup the same files are refused with exit code 2."""
import importlib
import os
import subprocess

import numpy as np
import pytest
import scipy.io
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

N = 45


def _run(args, env):
    hostio = importlib.import_module("pem_spgemm_amd.hostio")
    return subprocess.run([hostio.CLI_PATH, *args], env=env, capture_output=True, text=True, timeout=120)


def _env(tmp_path):
    return dict(os.environ, PEM_CSV=str(tmp_path / "r.csv"), PEM_REPEAT="2")


def _write(path, symmetry, I, J, V):
    with open(path, "w") as f:
        f.write(f"%%MatrixMarket matrix coordinate real {symmetry}\n{N} {N} {len(I)}\n")
        for i, j, v in zip(I, J, V):
            f.write(f"{i + 1} {j + 1} {v:.1f}\n")


def _square(I, J, V):
    """A*A of the matrix whose duplicates are summed, canonical; small integers: every sum and product is exact"""
    A = sp.coo_matrix((V, (I, J)), shape=(N, N)).tocsr()
    C = (A @ A).tocsr()
    C.sort_indices()
    return C


def _same(path, want, A_nnz, stdout):
    C = scipy.io.mmread(path).tocsr()
    C.sort_indices()
    assert C.shape == want.shape and (C != want).nnz == 0
    # the product keeps the entries that cancel to zero; scipy's does too (no eliminate_zeros): the patterns agree
    assert np.array_equal(C.indptr, want.indptr) and np.array_equal(C.indices, want.indices) and np.array_equal(C.data, want.data)
    assert f"Nnz: {A_nnz}\n" in stdout


@pytest.fixture
def general(tmp_path):
    rng = np.random.default_rng(71)
    key = rng.choice(N * N, 260, replace=False)
    key = np.concatenate([key, key[rng.integers(0, 260, 140)]])[rng.permutation(400)]
    I, J, V = key // N, key % N, rng.integers(1, 5, 400).astype(np.float64)
    path = str(tmp_path / "dups.mtx")
    _write(path, "general", I, J, V)
    return path, I, J, V


@pytest.mark.parametrize("fp32", (False, True), ids=("f64", "f32"))
def test_dup_plus_sums_the_duplicates(general, tmp_path, fp32):
    path, I, J, V = general
    fc = str(tmp_path / "C.mtx")
    out = _run([path, "0", "--dup", "plus", "--out", fc] + (["--fp32"] if fp32 else []), _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    _same(fc, _square(I, J, V), 260, out.stdout)


def test_symmetric_file_listing_both_triangles(tmp_path):
    rng = np.random.default_rng(72)
    key = rng.choice(N * N, 150, replace=False)
    I, J = key // N, key % N
    I, J = np.concatenate([I, J]), np.concatenate([J, I])          # both triangles (the diagonal entries twice)
    V = rng.integers(1, 5, len(I)).astype(np.float64)
    path, fc = str(tmp_path / "sym.mtx"), str(tmp_path / "C.mtx")
    _write(path, "symmetric", I, J, V)
    out = _run([path, "0", "--dup", "plus", "--out", fc], _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    off = I != J                                                   # the reader's expansion: every off-diagonal line also mirrored
    eI, eJ, eV = np.concatenate([I, J[off]]), np.concatenate([J, I[off]]), np.concatenate([V, V[off]])
    A = sp.coo_matrix((eV, (eI, eJ)), shape=(N, N)).tocsr()
    _same(fc, _square(eI, eJ, eV), A.nnz, out.stdout)
    refused = _run([path, "0", "--out", fc + ".no"], _env(tmp_path))
    assert refused.returncode == 2 and not os.path.exists(fc + ".no")
    assert f"conversion of {path} failed" in refused.stderr and "duplicate (row, col) entries" in refused.stderr


def test_without_dup_duplicates_are_still_refused(general, tmp_path):
    path, _, _, _ = general
    fc = str(tmp_path / "C.mtx")
    out = _run([path, "0", "--out", fc], _env(tmp_path))
    assert out.returncode == 2, out.stdout + out.stderr
    assert f"pemspgemm: conversion of {path} failed: duplicate (row, col) entries in the input" in out.stderr
    assert not os.path.exists(fc)
