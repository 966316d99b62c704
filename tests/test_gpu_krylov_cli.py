"""GPU: `pemspgemm A.mtx 0 --solve cg|bicgstab --rhs b.mtx [--precond none|jacobi|ilu0] [--rtol R] [--max-iters N] --out x.mtx` (the
Krylov solve on the final result, C = A*A) against Tiled.solve of the same result built through the Python binding, compared the
way test_gpu_trsv_cli.py compares its vector; the report line, --fp32, and the refusals that need the device."""
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


def _matrix(seed=71):
    """200 rows, symmetric: a diagonal of 2 .. 3 plus 450 mirrored entries below 0.02, so that C = A*A is symmetric positive definite
    and stores its diagonal"""
    rng = np.random.default_rng(seed)
    key = np.sort(rng.choice(N * N, 450, replace=False))
    I, J = key // N, key % N
    lower = I > J
    I, J = I[lower], J[lower]
    V = rng.uniform(-0.02, 0.02, len(I))
    d = rng.uniform(2.0, 3.0, N)
    return (np.concatenate([I, J, np.arange(N)]).astype(np.int32), np.concatenate([J, I, np.arange(N)]).astype(np.int32),
            np.concatenate([V, V, d]))


@pytest.fixture
def mats(standins, tmp_path):
    I, J, V = _matrix()
    fa, fb = str(tmp_path / "A.mtx"), str(tmp_path / "b.mtx")
    standins.write_mtx(fa, N, N, I, J, V)
    b = np.random.default_rng(72).standard_normal(N)
    _write_vector(fb, b)
    return fa, fb, (I, J, V), b


def _expected(pkg, ctx, coo, b, dtype, method, precond, **kw):
    A = pkg.Tiled.from_coo(ctx, N, N, *coo, dtype=dtype)
    p = pkg.CPlan(ctx, A, A)
    p.spgemm()
    R = pkg.Tiled.from_cplan(p)
    x, info = R.solve(torch.from_numpy(np.asarray(b, dtype)).cuda(), method=method, precond=precond, **kw)
    torch.cuda.synchronize()
    return x.cpu().numpy(), info


def _same(got, want):
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    return got.shape == want.shape and bool(np.all((got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want))))


@pytest.mark.parametrize("fp32", (False, True), ids=("f64", "f32"))
@pytest.mark.parametrize("method,precond", [("cg", None), ("cg", "jacobi"), ("cg", "ilu0"), ("bicgstab", "none"), ("bicgstab", "ilu0")])
def test_solve_matches_tiled_solve(pkg, ctx, mats, tmp_path, method, precond, fp32):
    fa, fb, coo, b = mats
    fx = str(tmp_path / "x.mtx")
    rtol = 1e-4 if fp32 else 1e-10
    args = [fa, "0", "--solve", method, "--rhs", fb, "--rtol", repr(rtol), "--max-iters", "50", "--out", fx]
    out = _run(args + (["--precond", precond] if precond else []) + (["--fp32"] if fp32 else []), _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    dt = np.float32 if fp32 else np.float64
    want, info = _expected(pkg, ctx, coo, b, dt, method, precond, rtol=rtol, max_iters=50)
    assert info["status"] == "converged" and info["iters"] > 0
    assert out.stdout.count("solve: ") == 1 and "solution written to" in out.stdout
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("solve: ")][0]
    assert line.startswith(f"solve: {method} with {precond or 'none'} of C: solve ") and f", {info['iters']} iterations, converged, " in line, line
    assert f"relative residual {np.sqrt(info['rr'] / info['bb']):.3e}" in line and f"{info['readbacks']} read-backs" in line, line
    assert _same(_read_vector(fx, dt), want)   # (17 / 9 significant digits: the round trip is exact)
    row = (tmp_path / "r.csv").read_text().strip().splitlines()[-1].split(",")
    assert len(row) == 22   # (the CSV row describes the product)


def test_max_iters_is_reported_not_refused(pkg, ctx, mats, tmp_path):
    fa, fb, coo, b = mats
    fx = str(tmp_path / "x.mtx")
    out = _run([fa, "0", "--solve", "cg", "--rhs", fb, "--rtol", "1e-14", "--max-iters", "2", "--out", fx], _env(tmp_path))
    assert out.returncode == 0 and ", 2 iterations, max_iters, " in out.stdout, out.stdout + out.stderr
    want, info = _expected(pkg, ctx, coo, b, np.float64, "cg", None, rtol=1e-14, max_iters=2)
    assert info["status"] == "max_iters" and _same(_read_vector(fx, np.float64), want)


def test_refusals_on_the_device(standins, mats, tmp_path):
    fa, fb, _, b = mats
    env = _env(tmp_path)
    short = str(tmp_path / "short.mtx")
    _write_vector(short, b[:-1])
    out = _run([fa, "0", "--solve", "cg", "--rhs", short], env)
    assert out.returncode == 1 and f"--rhs {short}: the vector has {N - 1} values; C has {N} rows. Exiting." in out.stdout, out.stdout
    # a result that is not square: C = A*B, 6 x 4 times 4 x 5
    f6, f4 = str(tmp_path / "A6.mtx"), str(tmp_path / "B4.mtx")
    standins.write_mtx(f6, 6, 4, np.arange(4, dtype=np.int32), np.arange(4, dtype=np.int32), np.ones(4))
    standins.write_mtx(f4, 4, 5, np.arange(4, dtype=np.int32), np.arange(4, dtype=np.int32), np.ones(4))
    out = _run([f6, "0", "--B", f4, "--solve", "bicgstab", "--rhs", fb], env)
    assert out.returncode == 1 and "--solve bicgstab: C is 6 x 5; a Krylov solver needs a square matrix. Exiting." in out.stdout, out.stdout + out.stderr
    # ilu0 of a result without a diagonal: the library's message
    out = _run([fa, "0", "--select", "offdiag", "--solve", "cg", "--precond", "ilu0", "--rhs", fb], env)
    assert out.returncode == 1 and "--precond ilu0: " in out.stdout and "no stored diagonal entry" in out.stdout, out.stdout + out.stderr
