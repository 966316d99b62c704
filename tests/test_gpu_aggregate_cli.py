"""GPU: `pemspgemm A.mtx 0 --aggregate SEED [--out agg.mtx]` (the MIS(2) aggregation of the final result's pattern on the device,
INTEGRATION.md section 3zb) against aggref on the same pattern -- C = A*A of a small golden .mtx, and the strict upper triangle of a
golden product (every edge stored one way) -- and its refusals, each one line and exit code 1."""
import importlib
import os
import subprocess

import numpy as np
import pytest
import torch

import aggref as ar

pytestmark = pytest.mark.gpu

torch.cuda.is_available()

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CAGE4 = os.path.join(GOLDEN, "mm_cage4_standin.mtx")


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


def _cage4_square():
    """(n, I, J): the structural pattern of C = A*A of the golden 9 x 9 file"""
    body = [ln.split() for ln in open(CAGE4).read().splitlines() if not ln.startswith("%")]
    n = int(body[0][0])
    P = np.zeros((n, n), np.int64)
    for i, j, _ in body[1:]:
        P[int(i) - 1, int(j) - 1] = 1
    I, J = np.nonzero(P @ P)
    return n, I.astype(np.int32), J.astype(np.int32)


def _rand300_upper(standins, tmp_path):
    """(file, n, I, J): the golden rand_300 input written out, and the strict upper triangle of its golden product's pattern"""
    z = np.load(os.path.join(GOLDEN, "spgemm_rand_300.npz"))
    n = int(z["rows"])
    fa = str(tmp_path / "rand_300.mtx")
    standins.write_mtx(fa, n, n, z["I"], z["J"], z["V"])
    I = np.repeat(np.arange(n, dtype=np.int32), np.diff(z["c_rowptr"]))
    J = np.asarray(z["c_colidx"], np.int32)
    up = J > I
    return fa, n, I[up], J[up]


@pytest.mark.parametrize("fp32", (False, True), ids=("f64", "f32"))
def test_aggregate_matches_the_model(tmp_path, fp32):
    n, I, J = _cage4_square()
    for seed in (12345, 0):
        fc = str(tmp_path / "agg.mtx")
        out = _run([CAGE4, "0", "--aggregate", str(seed), "--out", fc] + (["--fp32"] if fp32 else []), _env(tmp_path))
        assert out.returncode == 0, out.stderr + out.stdout
        agg, _, nc, rounds = ar.aggregate(n, I, J, seed=seed)
        assert out.stdout.count("aggregate: ") == 1, out.stdout
        assert f"aggregate: seed {seed} of C: {nc} aggregates in {rounds} rounds, {n} vertices, " in out.stdout, out.stdout
        assert "aggregates written to" in out.stdout
        assert np.array_equal(_read_ints(fc), agg + 1)
        row = (tmp_path / "r.csv").read_text().strip().splitlines()[-1].split(",")
        assert len(row) == 22   # (the CSV row keeps its width: it describes the product)


def test_after_select_and_without_out(standins, tmp_path):
    fa, n, I, J = _rand300_upper(standins, tmp_path)
    assert len(I) > 1000
    fc = str(tmp_path / "agg.mtx")
    agg, _, nc, rounds = ar.aggregate(n, I, J, seed=12345)
    assert nc > 1 and agg.min() == 0
    out = _run([fa, "0", "--select", "triu:1", "--aggregate", "12345", "--out", fc], _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    assert f"aggregate: seed 12345 of the selection: {nc} aggregates in {rounds} rounds, {n} vertices, " in out.stdout, out.stdout
    assert np.array_equal(_read_ints(fc), agg + 1)
    out = _run([fa, "0", "--select", "triu:1", "--aggregate", "12345"], _env(tmp_path))
    assert out.returncode == 0 and f"aggregate: seed 12345 of the selection: {nc} aggregates in {rounds} rounds" in out.stdout
    assert "written" not in out.stdout


def test_refusals(standins, tmp_path):
    env = _env(tmp_path)
    fx = str(tmp_path / "X.mtx")   # (a well-formed dense operand: the refusal is the combination's, not the file's)
    with open(fx, "w") as f:
        f.write("%%MatrixMarket matrix array real general\n9 1\n" + "1.0\n" * 9)
    frect = str(tmp_path / "R.mtx")
    standins.write_mtx(frect, 9, 4, np.array([0, 3, 8], np.int32), np.array([0, 1, 3], np.int32), np.ones(3))
    lines = [(["--aggregate", bad], f"--aggregate {bad}: want a seed in 0 .. 4294967295. Exiting.") for bad in ("x", "", "-1", "1.5", "4294967296")]
    for other, more in (("--gpus", ["2"]), ("--power", ["3"]), ("--reduce", ["rows"]), ("--bfs", ["1"]), ("--argreduce", ["rows:min"]),
                        ("--bfs-parents", ["1"]), ("--trsv", ["lower"]), ("--spmm", [fx]), ("--sddmm", [fx]), ("--colour", ["3"]),
                        ("--colour-natural", []), ("--components", [])):
        lines.append((["--aggregate", "7", other] + more, f"--aggregate does not combine with {other}. Exiting."))
    for args, line in lines:
        out = _run([CAGE4, "0"] + args, env)
        assert out.returncode == 1 and out.stdout == line + "\n", (args, out.stdout, out.stderr)
    assert not os.path.exists(tmp_path / "r.csv")
    out = _run([CAGE4, "0", "--B", frect, "--aggregate", "7"], env)   # C = A * B is 9 x 4: known only once the result exists
    assert out.returncode == 1 and out.stdout.splitlines()[-1] == "--aggregate: C is 9 x 4; an aggregation needs a square matrix. Exiting.", out.stdout
