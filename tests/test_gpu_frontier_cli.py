"""GPU: `pemspgemm A.mtx 0 --bfs SRC [--out levels.mtx]` (a breadth-first search over the final result on the device) against
frontierref's BFS of the same result exported through the Python binding; and its refusals."""
import importlib
import os
import subprocess

import numpy as np
import pytest
import torch

import frontierref as fr

pytestmark = pytest.mark.gpu

torch.cuda.is_available()

N = 150


def _run(args, env):
    hostio = importlib.import_module("pem_spgemm_amd.hostio")
    return subprocess.run([hostio.CLI_PATH, *args], env=env, capture_output=True, text=True, timeout=120)


def _env(tmp_path, name="r.csv"):
    return dict(os.environ, PEM_CSV=str(tmp_path / name), PEM_REPEAT="2")


def _read_levels(path):
    lines = open(path).read().splitlines()
    assert lines[0].split() == ["%%MatrixMarket", "matrix", "array", "integer", "general"]
    body = [ln for ln in lines if not ln.startswith("%")]
    assert body[0].split() == [str(len(body) - 1), "1"]
    return np.array([int(x) for x in body[1:]], np.int32)


@pytest.fixture
def mats(standins, tmp_path):
    """a sparse digraph whose square still leaves vertices unreachable (a third of the vertices have no out-edges, some no in-edges)"""
    rng = np.random.default_rng(53)
    key = np.sort(rng.choice(N * N, 260, replace=False))
    I, J = (key // N).astype(np.int32), (key % N).astype(np.int32)
    keep = (I % 3 != 1) & (J % 11 != 4)
    I, J = I[keep], J[keep]
    V = rng.uniform(-1, 1, len(I))
    fa, fr_ = str(tmp_path / "A.mtx"), str(tmp_path / "R.mtx")
    standins.write_mtx(fa, N, N, I, J, V)
    standins.write_mtx(fr_, N, 60, I[J < 60], J[J < 60], V[J < 60])
    return fa, fr_, (I, J, V)


def _product_csr(pkg, ctx, coo, dtype):
    A = pkg.Tiled.from_coo(ctx, N, N, *coo, dtype=dtype)
    p = pkg.CPlan(ctx, A, A)
    p.spgemm()
    rp, ci, _ = p.export_csr()
    return rp.astype(np.int64), ci.astype(np.int64)


@pytest.mark.parametrize("fp32", (False, True), ids=("f64", "f32"))
def test_bfs_levels_match_the_model(pkg, ctx, mats, tmp_path, fp32):
    fa, _, coo = mats
    rp, ci = _product_csr(pkg, ctx, coo, np.float32 if fp32 else np.float64)
    src = int(np.argmax(np.diff(rp)))
    fl = str(tmp_path / "levels.mtx")
    out = _run([fa, "0", "--bfs", str(src + 1), "--out", fl] + (["--fp32"] if fp32 else []), _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    want, depth, reached = fr.bfs(N, rp, ci, src)
    assert 1 < reached < N and depth >= 2   # (the case has levels and unreachable vertices)
    assert out.stdout.count("bfs: ") == 1 and f"bfs: from {src + 1} over C: depth {depth}, reached {reached} of {N}" in out.stdout, out.stdout
    assert "levels written to" in out.stdout
    assert np.array_equal(_read_levels(fl), want)
    row = (tmp_path / "r.csv").read_text().strip().splitlines()[-1].split(",")
    assert len(row) == 22   # (the CSV row keeps its width: it describes the product)


def test_bfs_after_select_and_without_out(pkg, ctx, mats, tmp_path):
    fa, _, coo = mats
    A = pkg.Tiled.from_coo(ctx, N, N, *coo)
    p = pkg.CPlan(ctx, A, A)
    p.spgemm()
    rp, ci, _ = pkg.Tiled.from_cplan(p).select("triu", 1).export_csr()
    src = int(np.argmax(np.diff(rp)))
    _, depth, reached = fr.bfs(N, rp.astype(np.int64), ci.astype(np.int64), src)
    assert depth >= 1
    out = _run([fa, "0", "--select", "triu:1", "--bfs", str(src + 1)], _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    assert f"bfs: from {src + 1} over the selection: depth {depth}, reached {reached} of {N}" in out.stdout and "written" not in out.stdout, out.stdout


def test_bfs_refusals(mats, tmp_path):
    fa, frect, _ = mats
    env = _env(tmp_path)
    for args, word in (([fa, "0", "--bfs", "1", "--gpus", "2"], "--gpus"), ([fa, "0", "--bfs", "1", "--power", "3"], "--power"),
                       ([fa, "0", "--bfs", "1", "--reduce", "rows"], "--reduce"), ([fa, "0", "--bfs", "0"], "1-based vertex"),
                       ([fa, "0", "--bfs", "-3"], "1-based vertex"), ([fa, "0", "--bfs", "x"], "1-based vertex"),
                       ([fa, "0", "--bfs", "2x"], "1-based vertex"), ([fa, "0", "--bfs", ""], "1-based vertex")):
        out = _run(args, env)
        assert out.returncode != 0 and word in out.stdout, (args, out.stdout, out.stderr)
    assert not os.path.exists(tmp_path / "r.csv")
    out = _run([fa, "0", "--bfs", str(N + 1)], env)       # known only once the result exists
    assert out.returncode != 0 and f"has {N} vertices" in out.stdout, out.stdout
    out = _run([fa, "0", "--B", frect, "--bfs", "1"], env)   # C = A * B is 150 x 60
    assert out.returncode != 0 and "a search needs a square matrix" in out.stdout, out.stdout
