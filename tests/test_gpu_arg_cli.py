"""GPU: `pemspgemm A.mtx 0 --argreduce rows|cols:min|max [--out idx.mtx]` and `--bfs-parents SRC [--out parents.mtx]` (arg folds of
the final result on the device) against argref on the same result exported through the Python binding;
and their refusals, each one line and exit code 1."""
import importlib
import os
import subprocess

import numpy as np
import pytest
import torch

import argref as ar

pytestmark = pytest.mark.gpu

torch.cuda.is_available()

N = 150


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


@pytest.fixture
def mats(standins, tmp_path):
    """a sparse digraph whose square still leaves vertices unreachable and rows empty; small integer values, so the products tie"""
    rng = np.random.default_rng(53)
    key = np.sort(rng.choice(N * N, 260, replace=False))
    I, J = (key // N).astype(np.int32), (key % N).astype(np.int32)
    keep = (I % 3 != 1) & (J % 11 != 4)
    I, J = I[keep], J[keep]
    V = rng.integers(-2, 3, len(I)).astype(np.float64)
    fa, fr_ = str(tmp_path / "A.mtx"), str(tmp_path / "R.mtx")
    standins.write_mtx(fa, N, N, I, J, V)
    standins.write_mtx(fr_, N, 60, I[J < 60], J[J < 60], V[J < 60])
    return fa, fr_, (I, J, V)


def _product_csr(pkg, ctx, coo, dtype):
    A = pkg.Tiled.from_coo(ctx, N, N, *coo, dtype=dtype)
    p = pkg.CPlan(ctx, A, A)
    p.spgemm()
    rp, ci, v = p.export_csr()
    return rp.astype(np.int64), ci.astype(np.int64), v


@pytest.mark.parametrize("fp32", (False, True), ids=("f64", "f32"))
@pytest.mark.parametrize("spec", ("rows:min", "rows:max", "cols:min", "cols:max"))
def test_argreduce_matches_the_model(pkg, ctx, mats, tmp_path, spec, fp32):
    fa, _, coo = mats
    dtype = np.float32 if fp32 else np.float64
    rp, ci, v = _product_csr(pkg, ctx, coo, dtype)
    dim, op = spec.split(":")
    fi = str(tmp_path / "idx.mtx")
    out = _run([fa, "0", "--argreduce", spec, "--out", fi] + (["--fp32"] if fp32 else []), _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    wy, widx = ar.reduce_arg(N, N, rp, ci, v, op, dtype, dim)
    assert (widx < 0).any() and (widx >= 0).sum() > 20   # (the case has empty lines)
    ties = sum(int(np.sum(v[rp[i]:rp[i + 1]] == wy[i]) > 1) for i in range(N)) if dim == "rows" else 1
    assert ties > 0   # (and lines whose best value sits in several places)
    assert out.stdout.count("argreduce: ") == 1, out.stdout
    assert f"argreduce: {dim} {op} of C: argreduce " in out.stdout and f"ms, {N} indices, {int((widx >= 0).sum())} lines with one" in out.stdout
    assert "indices written to" in out.stdout
    assert np.array_equal(_read_ints(fi), widx + 1)
    row = (tmp_path / "r.csv").read_text().strip().splitlines()[-1].split(",")
    assert len(row) == 22   # (the CSV row keeps its width: it describes the product)


@pytest.mark.parametrize("fp32", (False, True), ids=("f64", "f32"))
def test_bfs_parents_match_the_model(pkg, ctx, mats, tmp_path, fp32):
    fa, _, coo = mats
    rp, ci, _ = _product_csr(pkg, ctx, coo, np.float32 if fp32 else np.float64)
    src = int(np.argmax(np.diff(rp)))
    fp = str(tmp_path / "parents.mtx")
    out = _run([fa, "0", "--bfs-parents", str(src + 1), "--out", fp] + (["--fp32"] if fp32 else []), _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    level, parent, depth, reached = ar.bfs_parents(N, rp, ci, src)
    assert 1 < reached < N and depth >= 2   # (the case has levels and unreachable vertices)
    assert (ar.candidate_parents(N, rp, ci, level)[level > 0] > 1).any()   # (and vertices with a choice of parent)
    assert out.stdout.count("bfs: ") == 1 and f"bfs: from {src + 1} over C: depth {depth}, reached {reached} of {N}" in out.stdout, out.stdout
    assert "parents written to" in out.stdout
    got = _read_ints(fp)
    assert np.array_equal(got, parent + 1) and got[src] == src + 1 and (got == 0).any()
    row = (tmp_path / "r.csv").read_text().strip().splitlines()[-1].split(",")
    assert len(row) == 22


def test_after_select_and_without_out(pkg, ctx, mats, tmp_path):
    fa, _, coo = mats
    A = pkg.Tiled.from_coo(ctx, N, N, *coo)
    p = pkg.CPlan(ctx, A, A)
    p.spgemm()
    rp, ci, v = pkg.Tiled.from_cplan(p).select("triu", 1).export_csr()
    rp, ci = rp.astype(np.int64), ci.astype(np.int64)
    src = int(np.argmax(np.diff(rp)))
    _, _, depth, reached = ar.bfs_parents(N, rp, ci, src)
    out = _run([fa, "0", "--select", "triu:1", "--bfs-parents", str(src + 1)], _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    assert f"bfs: from {src + 1} over the selection: depth {depth}, reached {reached} of {N}" in out.stdout and "written" not in out.stdout, out.stdout
    _, widx = ar.reduce_arg(N, N, rp, ci, v, "max", np.float64, "rows")
    out = _run([fa, "0", "--select", "triu:1", "--argreduce", "rows:max"], _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    assert "argreduce: rows max of the selection: argreduce " in out.stdout and f"{int((widx >= 0).sum())} lines with one" in out.stdout
    assert "written" not in out.stdout


def test_refusals(mats, tmp_path):
    fa, frect, _ = mats
    env = _env(tmp_path)
    fx = str(tmp_path / "X.mtx")   # (a well-formed dense operand: the refusal is the combination's, not the file's)
    with open(fx, "w") as f:
        f.write("%%MatrixMarket matrix array real general\n" + f"{N} 1\n" + "1.0\n" * N)
    for args, line in (
            (["--argreduce", "rows:min", "--gpus", "2"], "--argreduce does not combine with --gpus. Exiting."),
            (["--argreduce", "rows:min", "--power", "3"], "--argreduce does not combine with --power. Exiting."),
            (["--argreduce", "rows:min", "--reduce", "rows"], "--argreduce does not combine with --reduce. Exiting."),
            (["--argreduce", "rows:min", "--bfs", "1"], "--argreduce does not combine with --bfs. Exiting."),
            (["--argreduce", "rows:min", "--spmm", fx], "--argreduce does not combine with --spmm. Exiting."),
            (["--argreduce", "rows:min", "--sddmm", fx], "--argreduce does not combine with --sddmm. Exiting."),
            (["--argreduce", "diag:min"], "--argreduce diag:min: unknown dimension diag (rows, cols). Exiting."),
            (["--argreduce", "rows"], "--argreduce rows: want rows|cols:min|max; unknown op  (min, max). Exiting."),
            (["--argreduce", "cols:plus"], "--argreduce cols:plus: want rows|cols:min|max; unknown op plus (min, max). Exiting."),
            (["--bfs-parents", "1", "--gpus", "2"], "--bfs-parents does not combine with --gpus. Exiting."),
            (["--bfs-parents", "1", "--power", "3"], "--bfs-parents does not combine with --power. Exiting."),
            (["--bfs-parents", "1", "--reduce", "rows"], "--bfs-parents does not combine with --reduce. Exiting."),
            (["--bfs-parents", "1", "--bfs", "1"], "--bfs-parents does not combine with --bfs. Exiting."),
            (["--bfs-parents", "1", "--argreduce", "rows:max"], "--bfs-parents does not combine with --argreduce. Exiting."),
            (["--bfs-parents", "1", "--spmm", fx], "--bfs-parents does not combine with --spmm. Exiting."),
            (["--bfs-parents", "1", "--sddmm", fx], "--bfs-parents does not combine with --sddmm. Exiting."),
            (["--bfs-parents", "0"], "--bfs-parents 0: want a 1-based vertex number. Exiting."),
            (["--bfs-parents", "-3"], "--bfs-parents -3: want a 1-based vertex number. Exiting."),
            (["--bfs-parents", "2x"], "--bfs-parents 2x: want a 1-based vertex number. Exiting."),
            (["--bfs-parents", ""], "--bfs-parents : want a 1-based vertex number. Exiting.")):
        out = _run([fa, "0"] + args, env)
        assert out.returncode == 1 and out.stdout == line + "\n", (args, out.stdout, out.stderr)
    assert not os.path.exists(tmp_path / "r.csv")
    out = _run([fa, "0", "--bfs-parents", str(N + 1)], env)       # known only once the result exists
    assert out.returncode == 1 and out.stdout.splitlines()[-1] == f"--bfs-parents {N + 1}: C has {N} vertices. Exiting.", out.stdout
    out = _run([fa, "0", "--B", frect, "--bfs-parents", "1"], env)   # C = A * B is 150 x 60
    assert out.returncode == 1 and out.stdout.splitlines()[-1] == "--bfs-parents 1: C is 150 x 60; a search needs a square matrix. Exiting.", out.stdout
