"""GPU: `pemspgemm A.mtx 0 --apply OP[:THUNK] [--row-scale r.mtx] [--col-scale c.mtx] [--scale-op OP] [--out C.mtx]` (the final
result's values changed on the device) against applyref on the plain run's --out, alone and with --semiring, --add, --select and
--fp32; and the length check that needs the result's shape."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import applyref as ap
import selectref as sel

pytestmark = pytest.mark.gpu

N, M = 150, 90


def _rand(rng, r, c, nz):
    key = np.sort(rng.choice(r * c, nz, replace=False))
    return (key // c).astype(np.int32), (key % c).astype(np.int32), rng.uniform(-1, 1, nz)


def _run(args, env):
    hostio = importlib.import_module("pem_spgemm_amd.hostio")
    return subprocess.run([hostio.CLI_PATH, *args], env=env, capture_output=True, text=True, timeout=120)


def _env(tmp_path, name="r.csv"):
    return dict(os.environ, PEM_CSV=str(tmp_path / name), PEM_REPEAT="2")


def _coo(path):
    import scipy.io
    C = scipy.io.mmread(path).tocsr()
    C.sort_indices()
    return np.repeat(np.arange(C.shape[0], dtype=np.int32), np.diff(C.indptr)), C.indices.astype(np.int32), C.data, C.shape


def _vector(path, v):
    with open(path, "w") as f:
        f.write("%%%%MatrixMarket matrix array real general\n%d 1\n" % len(v))
        f.writelines("%.17g\n" % x for x in v)
    return str(path)


@pytest.fixture
def mats(standins, tmp_path):
    rng = np.random.default_rng(47)
    fa, fb, fd = str(tmp_path / "A.mtx"), str(tmp_path / "B.mtx"), str(tmp_path / "D.mtx")
    standins.write_mtx(fa, N, N, *_rand(rng, N, N, 1200))
    standins.write_mtx(fb, N, M, *_rand(rng, N, M, 900))           # C = A*B is N x M: the two vectors differ in length
    standins.write_mtx(fd, N, M, *_rand(rng, N, M, 1500))
    r, c = rng.uniform(-2, 2, N), rng.uniform(-2, 2, M)
    return dict(A=fa, B=fb, D=fd, r=r, c=c, fr=_vector(tmp_path / "r.mtx", r), fc=_vector(tmp_path / "c.mtx", c))


def _plain(mats, tmp_path, extra, dt):
    """the run without the new stages: its --out is what they start from"""
    f0 = str(tmp_path / "C0.mtx")
    out = _run([mats["A"], "0", "--B", mats["B"], *extra, "--out", f0], _env(tmp_path, "r0.csv"))
    assert out.returncode == 0, out.stderr + out.stdout
    I, J, V, shape = _coo(f0)
    assert shape == (N, M)
    return I, J, V.astype(dt)


def _same(path, I, J, V, dt):
    gI, gJ, gV, _ = _coo(path)
    assert np.array_equal(gI, I) and np.array_equal(gJ, J)
    assert np.array_equal(gV.astype(dt).view(np.uint8), np.asarray(V, dt).view(np.uint8))


@pytest.mark.parametrize("fp32", (False, True), ids=("f64", "f32"))
def test_apply_and_scale_match_applyref(mats, tmp_path, fp32):
    dt = np.float32 if fp32 else np.float64
    f32 = ["--fp32"] if fp32 else []
    fc = str(tmp_path / "C.mtx")
    env = _env(tmp_path)
    I, J, V = _plain(mats, tmp_path, f32, dt)
    r, c = mats["r"].astype(dt), mats["c"].astype(dt)
    out = _run([mats["A"], "0", "--B", mats["B"], "--apply", "abs", "--out", fc] + f32, env)
    assert out.returncode == 0, out.stderr + out.stdout
    assert out.stdout.count("apply: abs:0 of C") == 1 and "scale: " not in out.stdout
    _same(fc, I, J, ap.apply(V, "abs"), dt)
    row = (tmp_path / "r.csv").read_text().strip().splitlines()[-1].split(",")
    assert len(row) == 22 and int(row[2]) == len(I)               # (the CSV row describes the product)
    out = _run([mats["A"], "0", "--B", mats["B"], "--apply", "powi:2", "--col-scale", mats["fc"], "--out", fc] + f32, env)
    assert out.returncode == 0, out.stderr + out.stdout
    assert "apply: powi:2 of C" in out.stdout and "scale: times of the applied matrix by columns" in out.stdout
    _same(fc, I, J, ap.scale(I, J, ap.apply(V, "powi", 2), None, c, "times"), dt)
    out = _run([mats["A"], "0", "--B", mats["B"], "--row-scale", mats["fr"], "--col-scale", mats["fc"], "--out", fc] + f32, env)
    assert out.returncode == 0, out.stderr + out.stdout
    _same(fc, I, J, ap.scale(I, J, V, r, c, "times"), dt)


def test_row_scale_plus_under_min_plus(mats, tmp_path):
    I, J, V = _plain(mats, tmp_path, ["--semiring", "min_plus"], np.float64)
    fc = str(tmp_path / "C.mtx")
    out = _run([mats["A"], "0", "--B", mats["B"], "--row-scale", mats["fr"], "--scale-op", "plus", "--semiring", "min_plus", "--out", fc], _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    assert "scale: plus of C by rows" in out.stdout
    _same(fc, I, J, ap.scale(I, J, V, mats["r"], None, "plus"), np.float64)


def test_with_add_and_select(mats, tmp_path):
    """the order of the stages: add, apply, scale, select"""
    I, J, V = _plain(mats, tmp_path, ["--add", mats["D"]], np.float64)
    fc = str(tmp_path / "C.mtx")
    out = _run([mats["A"], "0", "--B", mats["B"], "--add", mats["D"], "--apply", "rminus:1", "--row-scale", mats["fr"], "--col-scale", mats["fc"],
                "--scale-op", "max", "--select", "abs_gt:0.5", "--out", fc], _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    assert "apply: rminus:1 of the sum" in out.stdout and "scale: max of the applied matrix by rows and columns" in out.stdout
    assert "select: abs_gt:0.5 of the scaled matrix" in out.stdout
    W = ap.scale(I, J, ap.apply(V, "rminus", 1.0), mats["r"], mats["c"], "max")
    _same(fc, *sel.select(I, J, W, "abs_gt", 0.5), np.float64)
    row = (tmp_path / "r.csv").read_text().strip().splitlines()[-1].split(",")
    assert len(row) == 22


def test_vector_of_the_wrong_length(mats, tmp_path):
    fc = str(tmp_path / "C.mtx")
    for flag, path, word in (("--row-scale", mats["fc"], "the result has 150 rows"), ("--col-scale", mats["fr"], "the result has 90 columns")):
        out = _run([mats["A"], "0", "--B", mats["B"], flag, path, "--out", fc], _env(tmp_path))
        assert out.returncode != 0 and flag in out.stdout and word in out.stdout, out.stdout + out.stderr
        assert not os.path.exists(fc)
