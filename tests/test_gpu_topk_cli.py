"""GPU: `pemspgemm A.mtx 0 --topk DIM:ORDER:K [--out C.mtx]` (the final result cut to its first K entries per row or column on the
device) against the oracle's product cut by topkref, alone, after --select and with --fp32."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import selectref as sel
import topkref as tk

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


def _coo_of(rp, ci, v):
    return np.repeat(np.arange(len(rp) - 1, dtype=np.int32), np.diff(rp)), np.asarray(ci, np.int32), np.asarray(v)


@pytest.fixture
def mat(standins, tmp_path):
    a = _rand(np.random.default_rng(47), N, N, 1200)
    fa = str(tmp_path / "A.mtx")
    standins.write_mtx(fa, N, N, *a)
    return fa, a


def _product(oracle, a, fp32):
    dt = np.float32 if fp32 else np.float64
    oa = oracle.Csr(N, N, a[0], a[1], a[2].astype(dt).astype(np.float64))
    return _coo_of(*oracle.csr_spgemm(oa, oa, f32=fp32).arrays()), dt


def _check(C, I, J, V, dt):
    assert np.array_equal(C.indices, J) and np.array_equal(np.diff(C.indptr), np.bincount(I, minlength=N))
    assert np.array_equal(C.data.astype(dt).view(np.uint8), np.asarray(V, dt).view(np.uint8))


@pytest.mark.parametrize("fp32", (False, True), ids=("f64", "f32"))
@pytest.mark.parametrize("spec", ("cols:largest:3", "rows:abs_largest:2", "rows:smallest:0", "cols:abs_largest:1000"))
def test_topk_matches_cut_oracle(mat, oracle, tmp_path, spec, fp32):
    fa, a = mat
    fc = str(tmp_path / "C.mtx")
    out = _run([fa, "0", "--topk", spec, "--out", fc] + (["--fp32"] if fp32 else []), _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    c, dt = _product(oracle, a, fp32)
    dim, order, k = spec.split(":")
    I, J, V = tk.select_topk(c[0], c[1], c[2], order, dim, int(k), dt)
    _check(_mtx(fc), I, J, V, dt)
    lines = re.findall(r"^topk: (\S+) of C: topk [0-9.]+ms, total [0-9.]+ms, nnz (\d+) of (\d+) kept$", out.stdout, re.M)
    assert lines == [(spec, str(len(I)), str(len(c[0])))], out.stdout
    row = (tmp_path / "r.csv").read_text().strip().splitlines()[-1].split(",")
    assert len(row) == 22 and int(row[2]) == len(c[0])   # (the CSV row keeps its width and describes the product)


def test_select_in_front_of_topk(mat, oracle, tmp_path):
    fa, a = mat
    fc = str(tmp_path / "C.mtx")
    out = _run([fa, "0", "--topk", "cols:largest:4", "--select", "abs_gt:0.1", "--out", fc], _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    assert out.stdout.index("select: ") < out.stdout.index("topk: ") and "topk: cols:largest:4 of the selection" in out.stdout
    c, dt = _product(oracle, a, False)
    s = sel.select(*c, "abs_gt", 0.1)
    I, J, V = tk.select_topk(*s, "largest", "cols", 4)
    _check(_mtx(fc), I, J, V, dt)
    assert f"nnz {len(I)} of {len(s[0])} kept" in out.stdout
