"""GPU: `pemspgemm A.mtx 0 --solve cg|bicgstab --amg smoothed|plain --rhs b.mtx --out x.mtx` (the solve on the final result, C = A*A,
preconditioned by the stage's own multigrid hierarchy) against Tiled.solve(precond=Amg(...)) of the same result built through the
Python binding, bit for bit, fp64 and --fp32; the `amg:` line and the `solve:` line."""
import numpy as np
import pytest
import torch

from test_gpu_krylov_cli import N, _env, _matrix, _read_vector, _run, _same, _write_vector

pytestmark = pytest.mark.gpu

torch.cuda.is_available()


@pytest.fixture
def mats(standins, tmp_path):
    I, J, V = _matrix()
    fa, fb = str(tmp_path / "A.mtx"), str(tmp_path / "b.mtx")
    standins.write_mtx(fa, N, N, I, J, V)
    b = np.random.default_rng(72).standard_normal(N)
    _write_vector(fb, b)
    return fa, fb, (I, J, V), b


@pytest.mark.parametrize("fp32", (False, True), ids=("f64", "f32"))
@pytest.mark.parametrize("method,kind", [("cg", "smoothed"), ("bicgstab", "plain")])
def test_solve_matches_tiled_solve(pkg, ctx, mats, tmp_path, method, kind, fp32):
    fa, fb, coo, b = mats
    fx = str(tmp_path / "x.mtx")
    rtol = 1e-4 if fp32 else 1e-10
    args = [fa, "0", "--solve", method, "--amg", kind, "--rhs", fb, "--rtol", repr(rtol), "--max-iters", "50", "--out", fx]
    out = _run(args + (["--fp32"] if fp32 else []), _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    dt = np.float32 if fp32 else np.float64
    A = pkg.Tiled.from_coo(ctx, N, N, *coo, dtype=dt)
    p = pkg.CPlan(ctx, A, A)
    p.spgemm()
    R = pkg.Tiled.from_cplan(p)
    M = pkg.Amg(R, smooth=kind == "smoothed", refreshable=False)   # the CLI's options are the binding's defaults
    x, info = R.solve(torch.from_numpy(np.asarray(b, dt)).cuda(), method=method, precond=M, rtol=rtol, max_iters=50)
    torch.cuda.synchronize()
    ai = M.info
    M.close()
    assert info["status"] == "converged" and info["iters"] > 0 and ai["levels"] >= 2
    assert out.stdout.count("amg: ") == 1 and out.stdout.count("solve: ") == 1 and "solution written to" in out.stdout
    amg = [ln for ln in out.stdout.splitlines() if ln.startswith("amg: ")][0]
    rows = ", ".join(str(r) for r in ai["rows"])
    assert amg.startswith(f"amg: {kind} of C: {ai['levels']} levels, rows {rows}, operator complexity {ai['operator_complexity']:.4f}, "
                          f"{ai['launches']} launches per cycle, setup "), amg
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("solve: ")][0]
    assert line.startswith(f"solve: {method} with amg of C: solve ") and f", {info['iters']} iterations, converged, " in line, line
    assert f"relative residual {np.sqrt(info['rr'] / info['bb']):.3e}" in line and f"{info['readbacks']} read-backs" in line, line
    assert _same(_read_vector(fx, dt), x.cpu().numpy())   # (17 / 9 significant digits: the round trip is exact)

