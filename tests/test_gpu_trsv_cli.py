"""GPU: `pemspgemm A.mtx 0 --trsv lower|upper[:unit] [--rhs b.mtx] [--out x.mtx]` (the triangular solve on the final result) against
Tiled.trsv of the same result built through the Python binding; the all-ones default of b, :unit, --fp32 and --select in front; and
its refusals."""
import importlib
import os
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

torch.cuda.is_available()

N = 200


def _run(args, env):
    hostio = importlib.import_module("pem_spgemm_amd.hostio")
    return subprocess.run([hostio.CLI_PATH, *args], env=env, capture_output=True, text=True, timeout=120)


def _env(tmp_path, name="r.csv"):
    return dict(os.environ, PEM_CSV=str(tmp_path / name), PEM_REPEAT="2")


def _read_vector(path, dtype):
    lines = [ln for ln in open(path).read().splitlines() if not ln.startswith("%")]
    assert lines[0].split()[1] == "1"
    n = int(lines[0].split()[0])
    v = np.array([float(x) for x in lines[1:]], np.float64)
    assert len(v) == n
    return v.astype(dtype)


def _write_vector(path, v):
    with open(path, "w") as f:
        f.write(f"%%MatrixMarket matrix array real general\n{len(v)} 1\n")
        f.writelines("%.17g\n" % x for x in v)


def _matrix(seed=61):
    """200 rows: a diagonal of 2 .. 3 in size plus 900 entries below 0.02 on both sides, so that C = A*A stores its diagonal and even
    its unit-diagonal solves contract"""
    rng = np.random.default_rng(seed)
    key = np.sort(rng.choice(N * N, 900, replace=False))
    I, J = key // N, key % N
    off = I != J
    I, J = I[off], J[off]
    V = rng.uniform(-0.02, 0.02, len(I))
    return (np.concatenate([I, np.arange(N)]).astype(np.int32), np.concatenate([J, np.arange(N)]).astype(np.int32),
            np.concatenate([V, rng.uniform(2.0, 3.0, N) * rng.choice([-1.0, 1.0], N)]))


@pytest.fixture
def mats(standins, tmp_path):
    I, J, V = _matrix()
    fa, fb = str(tmp_path / "A.mtx"), str(tmp_path / "b.mtx")
    standins.write_mtx(fa, N, N, I, J, V)
    b = np.random.default_rng(62).standard_normal(N)
    _write_vector(fb, b)
    return fa, fb, (I, J, V), b


def _expected(pkg, ctx, coo, b, dtype, uplo, unit, select=None):
    A = pkg.Tiled.from_coo(ctx, N, N, *coo, dtype=dtype)
    p = pkg.CPlan(ctx, A, A)
    p.spgemm()
    R = pkg.Tiled.from_cplan(p)
    if select is not None:
        R = R.select(*select)
    x = R.trsv(torch.from_numpy(np.asarray(b, dtype)).cuda(), uplo, unit)
    info = R.trsv_info(uplo)
    torch.cuda.synchronize()
    ctx.synchronize()
    return x.cpu().numpy(), info


def _same(got, want):
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    return got.shape == want.shape and bool(np.all((got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want))))


@pytest.mark.parametrize("fp32", (False, True), ids=("f64", "f32"))
@pytest.mark.parametrize("spec", ("lower", "upper", "lower:unit", "upper:unit"))
def test_trsv_matches_tiled_trsv(pkg, ctx, mats, tmp_path, spec, fp32):
    fa, fb, coo, b = mats
    fx = str(tmp_path / "x.mtx")
    out = _run([fa, "0", "--trsv", spec, "--rhs", fb, "--out", fx] + (["--fp32"] if fp32 else []), _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    dt = np.float32 if fp32 else np.float64
    uplo, _, unit = spec.partition(":")
    want, info = _expected(pkg, ctx, coo, b, dt, uplo, unit == "unit")
    assert out.stdout.count("trsv: ") == 1 and "solution written to" in out.stdout
    assert f"trsv: {spec} of C: solve " in out.stdout and f"{info['levels']} levels, {info['launches']} launches" in out.stdout, out.stdout
    assert np.all(np.isfinite(want))
    assert _same(_read_vector(fx, dt), want), spec   # (17 / 9 significant digits: the round trip is exact)
    row = (tmp_path / "r.csv").read_text().strip().splitlines()[-1].split(",")
    assert len(row) == 22   # (the CSV row describes the product)


def test_default_rhs_is_all_ones_and_select_comes_first(pkg, ctx, mats, tmp_path):
    fa, _, coo, _ = mats
    fx = str(tmp_path / "x.mtx")
    out = _run([fa, "0", "--trsv", "lower", "--out", fx], _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    want, _ = _expected(pkg, ctx, coo, np.ones(N), np.float64, "lower", False)
    assert _same(_read_vector(fx, np.float64), want)
    out = _run([fa, "0", "--select", "offdiag", "--trsv", "upper:unit", "--out", fx], _env(tmp_path))
    assert out.returncode == 0 and "trsv: upper:unit of the selection" in out.stdout, out.stderr + out.stdout
    want, info = _expected(pkg, ctx, coo, np.ones(N), np.float64, "upper", True, select=("offdiag", 0))
    assert info["missing_diag"] == N and _same(_read_vector(fx, np.float64), want)
    out = _run([fa, "0", "--trsv", "upper"], _env(tmp_path))
    assert out.returncode == 0 and "trsv: upper of C" in out.stdout and "written" not in out.stdout, out.stdout


def test_trsv_refusals(standins, mats, tmp_path):
    fa, fb, _, b = mats
    env = _env(tmp_path)
    for args, word in (([fa, "0", "--trsv", "lower", "--gpus", "2"], "--trsv does not combine with --gpus"),
                       ([fa, "0", "--trsv", "upper", "--power", "3"], "--trsv does not combine with --power"),
                       ([fa, "0", "--trsv", "diag"], "unknown triangle diag (lower, upper)"),
                       ([fa, "0", "--trsv", "lower:unity"], "want lower|upper[:unit]"),
                       ([fa, "0", "--rhs", fb], "--rhs needs --trsv")):
        out = _run(args, env)
        assert out.returncode == 1 and word in out.stdout, (args, out.stdout, out.stderr)
    assert not os.path.exists(tmp_path / "r.csv")
    short = str(tmp_path / "short.mtx")
    _write_vector(short, b[:-1])
    out = _run([fa, "0", "--trsv", "lower", "--rhs", short], env)
    assert out.returncode == 1 and f"--rhs {short}: the vector has {N - 1} values; C has {N} rows. Exiting." in out.stdout, out.stdout
    # a result that is not square: C = A*B, 6 x 4 times 4 x 5
    f6, f4 = str(tmp_path / "A6.mtx"), str(tmp_path / "B4.mtx")
    standins.write_mtx(f6, 6, 4, np.arange(4, dtype=np.int32), np.arange(4, dtype=np.int32), np.ones(4))
    standins.write_mtx(f4, 4, 5, np.arange(4, dtype=np.int32), np.arange(4, dtype=np.int32), np.ones(4))
    out = _run([f6, "0", "--B", f4, "--trsv", "upper"], env)
    assert out.returncode == 1 and "--trsv upper: C is 6 x 5; a triangular solve needs a square matrix. Exiting." in out.stdout, out.stdout + out.stderr
    # a missing diagonal surfaces the library's message: the selection stores no diagonal entry
    out = _run([fa, "0", "--select", "offdiag", "--trsv", "lower"], env)
    assert out.returncode == 1 and "--trsv lower: pem_tiled_trsv: row 1 has no stored diagonal entry" in out.stdout, out.stdout + out.stderr
