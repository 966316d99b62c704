"""GPU: `pemspgemm A.mtx 0 --reduce rows|cols[:OP] [--out y.mtx]` (the final result folded on the device) against Tiled.reduce of the
same result built through the Python binding -- alone and with --semiring, --add, --select and --fp32; and its refusals."""
import importlib
import os
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

torch.cuda.is_available()

N = 150


def _rand(rng, r, c, nz):
    key = np.sort(rng.choice(r * c, nz, replace=False))
    return (key // c).astype(np.int32), (key % c).astype(np.int32), rng.uniform(-1, 1, nz)


def _run(args, env):
    hostio = importlib.import_module("pem_spgemm_amd.hostio")
    return subprocess.run([hostio.CLI_PATH, *args], env=env, capture_output=True, text=True, timeout=120)


def _env(tmp_path, name="r.csv"):
    return dict(os.environ, PEM_CSV=str(tmp_path / name), PEM_REPEAT="2")


def _read_coo(path):
    import scipy.io
    M = scipy.io.mmread(path).tocoo()
    return M.row.astype(np.int32), M.col.astype(np.int32), M.data.astype(np.float64)


def _read_vector(path, dtype):
    lines = [ln for ln in open(path).read().splitlines() if not ln.startswith("%")]
    assert lines[0].split()[1] == "1"
    n = int(lines[0].split()[0])
    v = np.array([float(x) for x in lines[1:]], np.float64)
    assert len(v) == n
    return v.astype(dtype)


@pytest.fixture
def mats(standins, tmp_path):
    rng = np.random.default_rng(47)
    a, d = _rand(rng, N, N, 1200), _rand(rng, N, N, 2000)
    # some empty rows and columns in A (they reduce to the identity)
    keep = (a[0] % 17 != 3) & (a[1] % 13 != 5)
    a = tuple(x[keep] for x in a)
    fa, fd = str(tmp_path / "A.mtx"), str(tmp_path / "D.mtx")
    standins.write_mtx(fa, N, N, *a)
    standins.write_mtx(fd, N, N, *d)
    return fa, fd


def _expected(pkg, ctx, fa, fd, dtype, semiring, op, dim, add=None, select=None):
    A = pkg.Tiled.from_coo(ctx, N, N, *_read_coo(fa), dtype=dtype)
    p = pkg.CPlan(ctx, A, A, semiring=semiring)
    p.spgemm()
    R = pkg.Tiled.from_cplan(p)
    if add is not None:
        D = pkg.Tiled.from_coo(ctx, N, N, *_read_coo(fd), dtype=dtype)
        R = pkg.Tiled.ewise(R, D, add[0], "union", add[1], add[2])
    if select is not None:
        R = R.select(*select)
    y = R.reduce(op, dim)
    torch.cuda.synchronize()
    ctx.synchronize()
    return y.cpu().numpy()


def _same(got, want):
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    return got.shape == want.shape and bool(np.all((got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want))))


@pytest.mark.parametrize("fp32", (False, True), ids=("f64", "f32"))
@pytest.mark.parametrize("spec", ("rows", "cols", "rows:max", "cols:min", "rows:times", "cols:lor", "rows:land", "cols:plus"))
def test_reduce_matches_tiled_reduce(pkg, ctx, mats, tmp_path, spec, fp32):
    fa, fd = mats
    fy = str(tmp_path / "y.mtx")
    out = _run([fa, "0", "--reduce", spec, "--out", fy] + (["--fp32"] if fp32 else []), _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    assert out.stdout.count("reduce: ") == 1 and "host sum" in out.stdout and "vector written to" in out.stdout
    dt = np.float32 if fp32 else np.float64
    dim, _, op = spec.partition(":")
    want = _expected(pkg, ctx, fa, fd, dt, "plus_times", op or "plus", dim)
    assert _same(_read_vector(fy, dt), want), spec
    row = (tmp_path / "r.csv").read_text().strip().splitlines()[-1].split(",")
    assert len(row) == 22   # (the CSV row describes the product)


@pytest.mark.parametrize("semiring,op", (("min_plus", "min"), ("max_times", "max"), ("lor_land", "lor"), ("plus_pair", "plus")))
def test_reduce_defaults_to_the_semirings_additive_op(pkg, ctx, mats, tmp_path, semiring, op):
    fa, fd = mats
    fy = str(tmp_path / "y.mtx")
    out = _run([fa, "0", "--semiring", semiring, "--reduce", "cols", "--out", fy], _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    assert f"reduce: cols {op} of C" in out.stdout
    assert _same(_read_vector(fy, np.float64), _expected(pkg, ctx, fa, fd, np.float64, semiring, op, "cols"))


def test_reduce_after_add_and_select(pkg, ctx, mats, tmp_path):
    fa, fd = mats
    fy = str(tmp_path / "y.mtx")
    out = _run([fa, "0", "--add", fd, "--alpha", "2", "--beta", "-0.5", "--select", "abs_gt:0.3", "--reduce", "rows:plus", "--out", fy],
               _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    assert "reduce: rows plus of the selection" in out.stdout
    want = _expected(pkg, ctx, fa, fd, np.float64, "plus_times", "plus", "rows", add=("plus", 2.0, -0.5), select=("abs_gt", 0.3))
    assert _same(_read_vector(fy, np.float64), want)
    out = _run([fa, "0", "--add", fd, "--reduce", "cols:max", "--out", fy], _env(tmp_path))
    assert out.returncode == 0 and "reduce: cols max of the sum" in out.stdout, out.stdout
    want = _expected(pkg, ctx, fa, fd, np.float64, "plus_times", "max", "cols", add=("plus", 1.0, 1.0))
    assert _same(_read_vector(fy, np.float64), want)


def test_reduce_without_out_prints_only(mats, tmp_path):
    out = _run([mats[0], "0", "--reduce", "rows"], _env(tmp_path))
    assert out.returncode == 0 and "reduce: rows plus of C" in out.stdout and "written" not in out.stdout, out.stdout


def test_reduce_refusals(mats, tmp_path):
    fa = mats[0]
    env = _env(tmp_path)
    for args, word in (([fa, "0", "--reduce", "rows", "--gpus", "2"], "--gpus"), ([fa, "0", "--reduce", "cols", "--power", "3"], "--power"),
                       ([fa, "0", "--reduce", "diag"], "unknown dimension"), ([fa, "0", "--reduce", "rows:minus"], "unknown op"),
                       ([fa, "0", "--reduce", "rows:"], "unknown op"), ([fa, "0", "--reduce", ""], "unknown dimension")):
        out = _run(args, env)
        assert out.returncode != 0 and word in out.stdout, (args, out.stdout, out.stderr)
    assert not os.path.exists(tmp_path / "r.csv")
