"""GPU: `pemspgemm A.mtx 0 --ilu0 [--trsv lower:unit --rhs b.mtx] [--out F.mtx]` (ILU(0) of the final result)
against Tiled.ilu0 of the same result built through the Python binding, and its refusals."""
import importlib
import os
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

torch.cuda.is_available()

N = 120


def _run(args, env):
    hostio = importlib.import_module("pem_spgemm_amd.hostio")
    return subprocess.run([hostio.CLI_PATH, *args], env=env, capture_output=True, text=True, timeout=120)


def _env(tmp_path):
    return dict(os.environ, PEM_CSV=str(tmp_path / "r.csv"), PEM_REPEAT="2")


def _matrix(seed=71):
    """120 rows: a diagonal of 2 .. 3 in size plus 500 small entries on both sides, so C = A*A stores its diagonal and dominates"""
    rng = np.random.default_rng(seed)
    key = np.sort(rng.choice(N * N, 500, replace=False))
    I, J = key // N, key % N
    off = I != J
    I, J = I[off], J[off]
    V = rng.uniform(-0.05, 0.05, len(I))
    return (np.concatenate([I, np.arange(N)]).astype(np.int32), np.concatenate([J, np.arange(N)]).astype(np.int32),
            np.concatenate([V, rng.uniform(2.0, 3.0, N) * rng.choice([-1.0, 1.0], N)]))


@pytest.fixture
def mats(standins, tmp_path):
    I, J, V = _matrix()
    fa, fb = str(tmp_path / "A.mtx"), str(tmp_path / "b.mtx")
    standins.write_mtx(fa, N, N, I, J, V)
    b = np.random.default_rng(72).standard_normal(N)
    with open(fb, "w") as f:
        f.write(f"%%MatrixMarket matrix array real general\n{N} 1\n")
        f.writelines("%.17g\n" % x for x in b)
    return fa, fb, (I, J, V), b


def _factor(pkg, ctx, coo, dtype):
    A = pkg.Tiled.from_coo(ctx, N, N, *coo, dtype=dtype)
    p = pkg.CPlan(ctx, A, A)
    p.spgemm()
    return pkg.Tiled.from_cplan(p).ilu0()


def _read_coo(path, dtype):
    lines = [ln for ln in open(path).read().splitlines() if not ln.startswith("%")]
    m, n, nnz = (int(x) for x in lines[0].split())
    rows = [ln.split() for ln in lines[1:]]
    assert len(rows) == nnz
    I, J = np.array([int(r[0]) - 1 for r in rows]), np.array([int(r[1]) - 1 for r in rows])
    V = np.array([float(r[2]) for r in rows], np.float64).astype(dtype)
    o = np.lexsort((J, I))
    return m, n, I[o], J[o], V[o]


def _same(got, want):
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    return got.shape == want.shape and bool(np.all((got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want))))


@pytest.mark.parametrize("fp32", (False, True), ids=("f64", "f32"))
def test_ilu0_out_and_lower_solve_match_the_binding(pkg, ctx, mats, tmp_path, fp32):
    fa, fb, coo, b = mats
    dt = np.float32 if fp32 else np.float64
    F = _factor(pkg, ctx, coo, dt)
    info = F.ilu0_info()
    rp, ci, v = F.export_csr()
    ff, fx = str(tmp_path / "F.mtx"), str(tmp_path / "x.mtx")
    out = _run([fa, "0", "--ilu0", "--out", ff] + (["--fp32"] if fp32 else []), _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    assert out.stdout.count("ilu0: of C: ilu0 ") == 1, out.stdout
    assert f"{info['levels']} levels, {info['launches']} launches, 0 zero pivots" in out.stdout, out.stdout
    m, n, I, J, V = _read_coo(ff, dt)
    assert (m, n) == (N, N) and np.array_equal(I, np.repeat(np.arange(N), np.diff(rp))) and np.array_equal(J, ci)
    assert np.all(np.isfinite(v)) and _same(V, v)   # (17 / 9 significant digits: the round trip is exact)
    row = (tmp_path / "r.csv").read_text().strip().splitlines()[-1].split(",")
    assert len(row) == 22   # (the CSV row describes the product)
    # L^-1 b: the vector stages see the factor
    out = _run([fa, "0", "--ilu0", "--trsv", "lower:unit", "--rhs", fb, "--out", fx] + (["--fp32"] if fp32 else []), _env(tmp_path))
    assert out.returncode == 0 and "trsv: lower:unit of the ILU(0) factor" in out.stdout, out.stderr + out.stdout
    want = F.trsv(torch.from_numpy(np.asarray(b, dt)).cuda(), "lower", unit_diag=True)
    torch.cuda.synchronize()
    ctx.synchronize()
    lines = [ln for ln in open(fx).read().splitlines() if not ln.startswith("%")]
    got = np.array([float(x) for x in lines[1:]], np.float64).astype(dt)
    assert _same(got, want.cpu().numpy())
    assert len((tmp_path / "r.csv").read_text().strip().splitlines()[-1].split(",")) == 22


def test_ilu0_refusals(standins, mats, tmp_path):
    fa, _, _, _ = mats
    env = _env(tmp_path)
    out = _run([fa, "0", "--ilu0", "--gpus", "2"], env)
    assert out.returncode == 1 and out.stdout == "--ilu0 does not combine with --gpus. Exiting.\n", (out.stdout, out.stderr)
    assert not os.path.exists(tmp_path / "r.csv")
    # a result that is not square: C = A*B, 6 x 4 times 4 x 5
    f6, f4 = str(tmp_path / "A6.mtx"), str(tmp_path / "B4.mtx")
    standins.write_mtx(f6, 6, 4, np.arange(4, dtype=np.int32), np.arange(4, dtype=np.int32), np.ones(4))
    standins.write_mtx(f4, 4, 5, np.arange(4, dtype=np.int32), np.arange(4, dtype=np.int32), np.ones(4))
    out = _run([f6, "0", "--B", f4, "--ilu0"], env)
    assert out.returncode == 1 and "--ilu0: C is 6 x 5; an incomplete LU needs a square matrix. Exiting." in out.stdout, out.stdout + out.stderr
    # a missing diagonal surfaces the library's message: the selection stores no diagonal entry
    out = _run([fa, "0", "--select", "offdiag", "--ilu0"], env)
    assert out.returncode == 1 and "--ilu0: pem_tiled_ilu0: row 1 has no stored diagonal entry" in out.stdout, out.stdout + out.stderr
