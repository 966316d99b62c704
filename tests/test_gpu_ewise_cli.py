"""GPU: `pemspgemm A.mtx 0 --add D.mtx [--alpha x] [--beta y] [--out C.mtx]` (C = alpha*(A*B) (+) beta*D on the device) against the
oracle + ewiseref, scipy and semiringref, and its refusals."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import ewiseref as er
import semiringref as sr

pytestmark = pytest.mark.gpu

N = 150


def _rand(rng, r, c, nz):
    key = np.sort(rng.choice(r * c, nz, replace=False))
    return (key // c).astype(np.int32), (key % c).astype(np.int32), rng.uniform(-1, 1, nz)


def _run(args, env):
    hostio = importlib.import_module("pem_spgemm_amd.hostio")
    return subprocess.run([hostio.CLI_PATH, *args], env=env, capture_output=True, text=True, timeout=120)


def _env(tmp_path, name="r.csv"):
    return dict(os.environ, PEM_CSV=str(tmp_path / name), PEM_REPEAT="2")


def _mtx(path):
    import scipy.io
    C = scipy.io.mmread(path).tocsr()
    C.sort_indices()
    return C


@pytest.fixture
def mats(standins, tmp_path):
    rng = np.random.default_rng(41)
    a, d = _rand(rng, N, N, 1200), _rand(rng, N, N, 2000)
    fa, fd = str(tmp_path / "A.mtx"), str(tmp_path / "D.mtx")
    standins.write_mtx(fa, N, N, *a)
    standins.write_mtx(fd, N, N, *d)
    return fa, fd, a, d


def _coo_of(rp, ci, v):
    return np.repeat(np.arange(len(rp) - 1, dtype=np.int32), np.diff(rp)), np.asarray(ci, np.int32), np.asarray(v)


@pytest.mark.parametrize("fp32", (False, True), ids=("f64", "f32"))
def test_add_matches_oracle_and_scipy(mats, oracle, tmp_path, fp32):
    import scipy.sparse as sp
    fa, fd, a, d = mats
    fc = str(tmp_path / "C.mtx")
    out = _run([fa, "0", "--add", fd, "--alpha", "2", "--beta", "-0.5", "--out", fc] + (["--fp32"] if fp32 else []), _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    assert out.stdout.count("add: C = ") == 1
    dt = np.float32 if fp32 else np.float64
    Va = a[2].astype(dt).astype(np.float64)
    oa = oracle.Csr(N, N, a[0], a[1], Va)
    c = _coo_of(*oracle.csr_spgemm(oa, oa, f32=fp32).arrays())
    I, J, V = er.ewise(N, (c[0], c[1], c[2].astype(dt)), (d[0], d[1], d[2].astype(dt)), "plus", "union", 2.0, -0.5)
    C = _mtx(fc)
    assert np.array_equal(C.indices, J) and np.array_equal(np.diff(C.indptr), np.bincount(I, minlength=N))
    assert np.array_equal(C.data.astype(dt), V)
    # and scipy's alpha*A*A + beta*D: same pattern, values to rounding
    A = sp.csr_matrix((Va, (a[0], a[1])), shape=(N, N))
    D = sp.csr_matrix((d[2].astype(dt).astype(np.float64), (d[0], d[1])), shape=(N, N))
    S = (2.0 * (A @ A) - 0.5 * D).tocsr()
    S.sort_indices()
    assert np.array_equal(S.indptr, C.indptr) and np.array_equal(S.indices, C.indices)
    assert np.allclose(S.data, C.data, rtol=1e-4 if fp32 else 1e-12, atol=1e-5 if fp32 else 1e-12)
    row = (tmp_path / "r.csv").read_text().strip().splitlines()[-1].split(",")
    assert len(row) == 22


def test_add_min_plus_matches_semiringref(mats, tmp_path):
    fa, fd, a, d = mats
    fc = str(tmp_path / "C.mtx")
    out = _run([fa, "0", "--semiring", "min_plus", "--add", fd, "--out", fc], _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    assert "min" in out.stdout
    ac = sr.coo_to_csr(N, N, *a)
    c = _coo_of(*sr.spgemm(ac, ac, N, "min_plus"))
    I, J, V = er.ewise(N, c, d, "min", "union")
    C = _mtx(fc)
    assert np.array_equal(C.indices, J) and np.array_equal(np.diff(C.indptr), np.bincount(I, minlength=N))
    assert sr.same_values(C.data, V)


def test_add_refusals(mats, standins, tmp_path):
    fa, fd = mats[0], mats[1]
    fsmall = str(tmp_path / "S.mtx")
    standins.write_mtx(fsmall, N, N - 1, np.array([0], np.int32), np.array([0], np.int32), np.array([1.0]))
    env = _env(tmp_path)
    for args, word in (([fa, "0", "--add", fd, "--gpus", "2"], "--gpus"), ([fa, "0", "--add", fd, "--mask", fa], "--mask"),
                       ([fa, "0", "--add", fd, "--power", "3"], "--power"),
                       ([fa, "0", "--add", fd, "--semiring", "min_plus", "--alpha", "2"], "plus_times"),
                       ([fa, "0", "--add", fd, "--semiring", "lor_land", "--beta", "0.5"], "plus_times"),
                       ([fa, "0", "--add", fsmall], "150 x 149")):
        out = _run(args, env)
        assert out.returncode != 0 and word in out.stdout, (args, out.stdout, out.stderr)
    assert not os.path.exists(tmp_path / "r.csv")
