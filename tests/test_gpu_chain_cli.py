"""GPU: `pemspgemm --power K` (A^K as K-1 chained products) against the plain run, the oracle and semiringref, and its refusals."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import semiringref as sr

pytestmark = pytest.mark.gpu


def _rand(rng, r, c, nz):
    key = rng.choice(r * c, nz, replace=False)
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
def amtx(standins, tmp_path):
    I, J, V = _rand(np.random.default_rng(31), 150, 150, 1200)
    fa = str(tmp_path / "A.mtx")
    standins.write_mtx(fa, 150, 150, I, J, V)
    return fa, I, J, V


def test_power_2_equals_the_plain_run(amtx, tmp_path):
    fa = amtx[0]
    outs = {}
    for label, extra in (("plain", []), ("power", ["--power", "2"])):
        out = _run([fa, "0", "--out", str(tmp_path / f"{label}.mtx")] + extra, _env(tmp_path, f"{label}.csv"))
        assert out.returncode == 0, out.stderr + out.stdout
        outs[label] = (tmp_path / f"{label}.mtx").read_bytes()
        if label == "power":
            assert "power: A^2 = A^1 * A" in out.stdout
    assert outs["plain"] == outs["power"]
    rows = [(tmp_path / f"{k}.csv").read_text().strip().splitlines()[-1].split(",") for k in ("plain", "power")]
    assert len(rows[0]) == len(rows[1]) and rows[0][1:3] == rows[1][1:3]   # flop count and C nnz


@pytest.mark.parametrize("fp32", (False, True), ids=("f64", "f32"))
def test_power_3_matches_the_oracle(amtx, oracle, tmp_path, fp32):
    fa, I, J, V = amtx
    fc = str(tmp_path / "C.mtx")
    out = _run([fa, "0", "--power", "3", "--out", fc] + (["--fp32"] if fp32 else []), _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    assert out.stdout.count("power: A^") == 2
    Vo = V.astype(np.float32).astype(np.float64) if fp32 else V
    a = oracle.Csr(150, 150, I, J, Vo)
    rp, ci, v = oracle.csr_spgemm(a, a, f32=fp32).arrays()
    c1 = oracle.Csr(150, 150, np.repeat(np.arange(150, dtype=np.int32), np.diff(rp)), ci, v)
    wrp, wci, wv = oracle.csr_spgemm(c1, a, f32=fp32).arrays()
    C = _mtx(fc)
    assert np.array_equal(C.indptr, wrp) and np.array_equal(C.indices, wci)
    assert np.array_equal(C.data, wv)
    row = (tmp_path / "r.csv").read_text().strip().splitlines()[-1].split(",")
    assert int(row[2]) == len(wci)                                    # the CSV row describes the last product


def test_power_3_lor_land_matches_semiringref(amtx, tmp_path):
    fa, I, J, V = amtx
    fc = str(tmp_path / "C.mtx")
    out = _run([fa, "0", "--power", "3", "--semiring", "lor_land", "--out", fc], _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    a = sr.coo_to_csr(150, 150, I, J, V)
    want = sr.spgemm(sr.spgemm(a, a, 150, "lor_land"), a, 150, "lor_land")
    C = _mtx(fc)
    assert np.array_equal(C.indptr, want[0]) and np.array_equal(C.indices, want[1]) and sr.same_values(C.data, want[2])


def test_power_refusals(amtx, tmp_path):
    fa = amtx[0]
    env = _env(tmp_path)
    for args, word in (([fa, "0", "--power", "1"], "at least 2"), ([fa, "0", "--power", "3", "--gpus", "2"], "--gpus"),
                       ([fa, "0", "--power", "3", "--mask", fa], "--mask"), ([fa, "0", "--power", "3", "--B", fa], "--B"),
                       ([fa, "0", "1", "--power", "3"], "A*A^T")):
        out = _run(args, env)
        assert out.returncode == 1 and word in out.stdout, (args, out.stdout)
    assert not os.path.exists(tmp_path / "r.csv")
