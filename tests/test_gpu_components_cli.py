"""GPU: `pemspgemm A.mtx 0 --components [--out labels.mtx]` (the connected components of the final result's pattern on the device,
INTEGRATION.md section 3za) against ccref on scipy's product pattern of a small .mtx the test writes; the CSV row keeps its width;
and the one refusal that needs the result: a matrix that is not square."""
import importlib
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import ccref as cc

pytestmark = pytest.mark.gpu

torch.cuda.is_available()


def _run(args, env):
    hostio = importlib.import_module("pem_spgemm_amd.hostio")
    return subprocess.run([hostio.CLI_PATH, *args], env=env, capture_output=True, text=True, timeout=120)


def _env(tmp_path, name="r.csv"):
    return dict(os.environ, PEM_CSV=str(tmp_path / name), PEM_REPEAT="2")


def _read_ints(path):
    lines = open(path).read().splitlines()
    assert lines[0].split() == ["%%MatrixMarket", "matrix", "array", "integer", "general"]
    body = [ln for ln in lines if not ln.startswith("%")]
    assert body[0].split() == [str(len(body) - 1), "1"]
    return np.array([int(x) for x in body[1:]], np.int32)


def _blocks():
    """(n, I, J): 90 vertices -- three paths stored one way on shuffled numbers (A*A joins every other vertex of a path, so each
    path falls into two components), a 4-clique and isolated vertices"""
    q = np.random.default_rng(90).permutation(90)
    I, J = [], []
    for lo, hi in ((0, 21), (21, 40), (40, 70)):
        I += q[lo:hi - 1].tolist()
        J += q[lo + 1:hi].tolist()
    k = q[70:74]
    I += [a for a in k for b in k]
    J += [b for a in k for b in k]
    return 90, np.array(I, np.int32), np.array(J, np.int32)


@pytest.mark.parametrize("fp32", (False, True), ids=("f64", "f32"))
def test_components_match_the_model(standins, tmp_path, fp32):
    n, I, J = _blocks()
    fa = str(tmp_path / "blocks.mtx")
    standins.write_mtx(fa, n, n, I, J, np.ones(len(I)))
    P = sp.coo_matrix((np.ones(len(I)), (I, J)), shape=(n, n)).tocsr()
    CI, CJ = (P @ P).nonzero()
    labels, rounds = cc.components_model(n, CI, CJ)
    assert np.array_equal(labels, cc.components_scipy(n, CI, CJ))
    nc = cc.ids_of(labels)[1]
    assert 20 < nc < 40 and rounds > 2
    fl = str(tmp_path / "labels.mtx")
    out = _run([fa, "0", "--components", "--out", fl] + (["--fp32"] if fp32 else []), _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    assert out.stdout.count("components: ") == 1 and f"components: {nc} components in {rounds} rounds, {n} vertices, " in out.stdout, out.stdout
    assert "labels written to" in out.stdout
    assert np.array_equal(_read_ints(fl), labels + 1)
    row = (tmp_path / "r.csv").read_text().strip().splitlines()[-1].split(",")
    assert len(row) == 22   # (the CSV row keeps its width: it describes the product)
    # without --out: the line, no file
    out = _run([fa, "0", "--components"], _env(tmp_path))
    assert out.returncode == 0 and f"components: {nc} components in {rounds} rounds" in out.stdout and "written" not in out.stdout


def test_a_result_that_is_not_square_is_refused(standins, tmp_path):
    fa = str(tmp_path / "A.mtx")
    standins.write_mtx(fa, 9, 9, np.arange(9, dtype=np.int32), np.arange(9, dtype=np.int32), np.ones(9))
    frect = str(tmp_path / "R.mtx")
    standins.write_mtx(frect, 9, 4, np.array([0, 3, 8], np.int32), np.array([0, 1, 3], np.int32), np.ones(3))
    out = _run([fa, "0", "--B", frect, "--components"], _env(tmp_path))   # C = A * B is 9 x 4: known only once the result exists
    assert out.returncode == 1 and out.stdout.splitlines()[-1] == "--components: C is 9 x 4; the components need a square matrix. Exiting.", out.stdout
