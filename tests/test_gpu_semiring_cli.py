"""GPU: `pemspgemm --semiring NAME` against the Python path (CPlan(..., semiring=NAME)), its refusals, and the default output
unchanged."""
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


@pytest.mark.parametrize("semiring", ["min_plus", "max_times", "plus_pair", "lor_land"])
@pytest.mark.parametrize("form", ["AB", "AAt", "A2_mask", "A2_fp32_mask_complement"])
def test_cli_semiring_matches_python(pkg, standins, ctx, tmp_path, form, semiring):
    import scipy.io
    rng = np.random.default_rng(23)
    m, k, n = 90, (60 if form in ("AB", "AAt") else 90), 75
    AI, AJ, AV = _rand(rng, m, k, 700)
    fa, fb, fm, fc = (str(tmp_path / f) for f in ("A.mtx", "B.mtx", "M.mtx", "C.mtx"))
    standins.write_mtx(fa, m, k, AI, AJ, AV)
    args = [fa, "0"]
    dtype = np.float32 if "fp32" in form else np.float64
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
    kw = {}
    if "mask" in form:
        MI, MJ, MV = _rand(rng, m, B.cols, m * B.cols // 4)
        standins.write_mtx(fm, m, B.cols, MI, MJ, MV)
        args += ["--mask", fm]
        kw = dict(mask=pkg.Tiled.from_coo(ctx, m, B.cols, MI, MJ, MV), complement="complement" in form)
        if kw["complement"]:
            args += ["--mask-complement"]
    if dtype == np.float32:
        args += ["--fp32"]
    args += ["--semiring", semiring, "--out", fc]
    out = _run(args, dict(os.environ, PEM_CSV=str(tmp_path / "r.csv"), PEM_REPEAT="2"))
    assert out.returncode == 0, out.stderr + out.stdout
    assert f"semiring {semiring}" in out.stdout
    plan = pkg.CPlan(ctx, A, B, semiring=semiring, **kw)
    plan.spgemm()
    rp, ci, v = plan.export_csr()
    Cf = scipy.io.mmread(fc).tocsr()
    Cf.sort_indices()
    assert Cf.shape == (m, B.cols) and np.array_equal(Cf.indptr, rp) and np.array_equal(Cf.indices, ci)
    assert np.array_equal(Cf.data, v.astype(np.float64))
    assert semiring in open(fc).read(4096)
    # the CSV row keeps its columns; the flop count stays the tile product's
    row = (tmp_path / "r.csv").read_text().strip().splitlines()[-1].split(",")
    assert int(row[1]) == pkg.flop_count(ctx, A, B)
    out2 = _run([a for a in args if a not in ("--semiring", semiring)], dict(os.environ, PEM_CSV=str(tmp_path / "r2.csv"), PEM_REPEAT="2"))
    assert out2.returncode == 0
    base_cols = len((tmp_path / "r2.csv").read_text().strip().splitlines()[-1].split(","))
    assert len(row) == base_cols


def test_cli_default_output_unchanged(standins, tmp_path):
    """without --semiring (and with --semiring plus_times) the result files and the .mtx are those of the plus-times product,
    byte for byte, and the report says nothing about semirings"""
    rng = np.random.default_rng(29)
    I, J, V = _rand(rng, 120, 120, 1500)
    fa = str(tmp_path / "A.mtx")
    standins.write_mtx(fa, 120, 120, I, J, V)
    outs = {}
    for label, extra in (("none", []), ("plus_times", ["--semiring", "plus_times"])):
        d = tmp_path / label
        d.mkdir()
        env = dict(os.environ, PEM_CSV=str(d / "r.csv"), PEM_REPEAT="1", PEM_RESULT_DIR=str(d))
        out = _run([fa, "1", "--out", str(d / "C.mtx")] + extra, env)
        assert out.returncode == 0, out.stderr + out.stdout
        assert "semiring" not in out.stdout
        files = sorted(f for f in os.listdir(d) if f.startswith("SPGEMM_RESULT") or f == "C.mtx")
        assert "C.mtx" in files and len(files) > 1
        outs[label] = {f: (d / f).read_bytes() for f in files}
    assert outs["none"] == outs["plus_times"]
    assert b"C = A*B by pemspgemm (pem-spgemm_amd)" in outs["none"]["C.mtx"]


def test_cli_semiring_refusals(standins, tmp_path):
    rng = np.random.default_rng(5)
    I, J, V = _rand(rng, 40, 40, 200)
    fa = str(tmp_path / "A.mtx")
    standins.write_mtx(fa, 40, 40, I, J, V)
    env = dict(os.environ, PEM_CSV=str(tmp_path / "r.csv"), PEM_REPEAT="1")
    out = _run([fa, "0", "--semiring", "min_plus", "--gpus", "2"], env)
    assert out.returncode == 1 and "--semiring" in out.stdout
    out = _run([fa, "0", "--semiring", "min_times"], env)
    assert out.returncode == 1 and "unknown semiring" in out.stdout
    assert not os.path.exists(tmp_path / "r.csv")
