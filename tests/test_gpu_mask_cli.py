"""GPU: `pemspgemm --mask M.mtx [--mask-complement]` against the Python path (CPlan(..., mask=M)), and its refusals."""
import importlib
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _rand(rng, r, c, nz):
    key = rng.choice(r * c, nz, replace=False)
    return (key // c).astype(np.int32), (key % c).astype(np.int32), rng.uniform(-1, 1, nz)


def _run(args, env):
    hostio = importlib.import_module("pem_spgemm_amd.hostio")
    return subprocess.run([hostio.CLI_PATH, *args], env=env, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("complement", [False, True])
@pytest.mark.parametrize("form", ["A2", "AB", "AAt", "A2_fp32"])
def test_cli_mask_matches_python(pkg, standins, ctx, tmp_path, complement, form):
    import scipy.io
    rng = np.random.default_rng(17)
    m, k, n = 90, (90 if form in ("A2", "A2_fp32") else 60), 75
    AI, AJ, AV = _rand(rng, m, k, 700)
    fa, fb, fm, fc = (str(tmp_path / f) for f in ("A.mtx", "B.mtx", "M.mtx", "C.mtx"))
    standins.write_mtx(fa, m, k, AI, AJ, AV)
    args = [fa, "0"]
    dtype = np.float32 if form == "A2_fp32" else np.float64
    A = pkg.Tiled.from_coo(ctx, m, k, AI, AJ, AV, dtype=dtype)
    if form == "AB":
        BI, BJ, BV = _rand(rng, k, n, 500)
        standins.write_mtx(fb, k, n, BI, BJ, BV)
        args += ["--B", fb]
        B = pkg.Tiled.from_coo(ctx, k, n, BI, BJ, BV)
    elif form == "AAt":
        args += ["1"]
        B = pkg.Tiled.from_coo(ctx, m, k, AI, AJ, AV, True)
    else:
        B = A
    if form == "A2_fp32":
        args += ["--fp32"]
    nc = B.cols
    MI, MJ, MV = _rand(rng, m, nc, m * nc // 4)
    standins.write_mtx(fm, m, nc, MI, MJ, MV)
    args += ["--mask", fm, "--out", fc] + (["--mask-complement"] if complement else [])
    out = _run(args, dict(os.environ, PEM_CSV=str(tmp_path / "r.csv"), PEM_REPEAT="2"))
    assert out.returncode == 0, out.stderr + out.stdout
    assert "count the unmasked product" in out.stdout
    M = pkg.Tiled.from_coo(ctx, m, nc, MI, MJ, MV)
    plan = pkg.CPlan(ctx, A, B, mask=M, complement=complement)
    plan.spgemm()
    rp, ci, v = plan.export_csr()
    Cf = scipy.io.mmread(fc).tocsr()
    Cf.sort_indices()
    assert Cf.shape == (m, nc) and np.array_equal(Cf.indptr, rp) and np.array_equal(Cf.indices, ci)
    assert np.array_equal(Cf.data, v.astype(np.float64))
    # the CSV row keeps its columns, flop = the unmasked count
    row = (tmp_path / "r.csv").read_text().strip().splitlines()[-1].split(",")
    assert int(row[1]) == pkg.flop_count(ctx, A, B)


def test_cli_mask_refusals(standins, tmp_path):
    rng = np.random.default_rng(5)
    I, J, V = _rand(rng, 40, 40, 200)
    fa, fm = str(tmp_path / "A.mtx"), str(tmp_path / "M.mtx")
    standins.write_mtx(fa, 40, 40, I, J, V)
    standins.write_mtx(fm, 40, 30, I[J < 30], J[J < 30], V[J < 30])
    env = dict(os.environ, PEM_CSV=str(tmp_path / "r.csv"), PEM_REPEAT="1")
    out = _run([fa, "0", "--mask", fa, "--gpus", "2"], env)
    assert out.returncode == 1 and "--mask" in out.stdout
    out = _run([fa, "0", "--mask", fm], env)                       # 40 x 30 mask, C is 40 x 40
    assert out.returncode == 1 and "40 x 30" in out.stdout
