"""GPU: `pemspgemm A.mtx 0 --sddmm X.mtx [--sddmm-y Y.mtx] [--out R.mtx]` (the final result's pattern with the values of X Y^T sampled
there, on the device) against sddmmref on the pattern of the same result built through the Python binding -- with and without
--sddmm-y, with --semiring, --fp32, after --select and for A*A^T; the sorted COO files; and its refusals."""
import importlib
import os
import subprocess

import numpy as np
import pytest
import torch

import sddmmref as sd

pytestmark = pytest.mark.gpu

torch.cuda.is_available()

N, M = 150, 110   # A is N x N; the A*A^T form takes an N x M matrix (its result is N x N too)


def _rand(rng, r, c, nz):
    key = np.sort(rng.choice(r * c, nz, replace=False))
    return (key // c).astype(np.int32), (key % c).astype(np.int32), rng.uniform(-1, 1, nz)


def _run(args, env):
    hostio = importlib.import_module("pem_spgemm_amd.hostio")
    return subprocess.run([hostio.CLI_PATH, *args], env=env, capture_output=True, text=True, timeout=120)


def _env(tmp_path):
    return dict(os.environ, PEM_CSV=str(tmp_path / "r.csv"), PEM_REPEAT="2", PEM_RESULT_DIR=str(tmp_path))


def _read_coo(path):
    import scipy.io
    A = scipy.io.mmread(path).tocoo()
    return A.row.astype(np.int32), A.col.astype(np.int32), A.data.astype(np.float64)


def _write_array(path, X, header="%%MatrixMarket matrix array real general"):
    with open(path, "w") as f:
        f.write(f"{header}\n% X\n{X.shape[0]} {X.shape[1]}\n")
        for v in X.T.ravel():   # column by column
            f.write(f"{float(v)!r}\n")


@pytest.fixture
def mats(standins, tmp_path):
    rng = np.random.default_rng(59)
    a, r = _rand(rng, N, N, 1500), _rand(rng, N, M, 1300)
    keep = (a[0] % 17 != 3) & (a[1] % 13 != 5)   # some empty rows and columns
    a = tuple(x[keep] for x in a)
    fa, fr = str(tmp_path / "A.mtx"), str(tmp_path / "R.mtx")
    standins.write_mtx(fa, N, N, *a)
    standins.write_mtx(fr, N, M, *r)
    return fa, fr


def _x(tmp_path, name, n, k, seed):
    # values exact in fp32, so the fp64 and fp32 runs read the same numbers
    X = np.random.default_rng(seed).uniform(-2, 2, (n, k)).astype(np.float32).astype(np.float64)
    X[::7, 0] = 0.0
    fx = str(tmp_path / name)
    _write_array(fx, X)
    return fx, X


def _pattern(pkg, ctx, path, dtype, aat=False, select=None):
    """the pattern of the CLI's final result, entries in CSR order"""
    rows, cols = (N, M) if aat else (N, N)
    A = pkg.Tiled.from_coo(ctx, rows, cols, *_read_coo(path), dtype=dtype)
    B = pkg.Tiled.from_coo(ctx, rows, cols, *_read_coo(path), transpose=True, dtype=dtype) if aat else A
    p = pkg.CPlan(ctx, A, B)
    p.spgemm()
    R = pkg.Tiled.from_cplan(p)
    if select is not None:
        R = R.select(*select)
    rp, ci, _ = R.export_csr()
    return sd.pattern_of(R.rows, rp, ci)


def _same(got, want, dtype):
    got, want = np.asarray(got).astype(dtype), np.asarray(want).astype(dtype)
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    return got.shape == want.shape and bool(np.all((got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want))))


@pytest.mark.parametrize("form", ("x_only", "x_and_y", "max_plus", "fp32", "select", "AAt"))
def test_sddmm_matches_the_reference(pkg, oracle, ctx, mats, tmp_path, form):
    fa, fr = mats
    fo = str(tmp_path / "out.mtx")
    k = 5
    fx, X = _x(tmp_path, "X.mtx", N, k, 3)
    fy, Y = _x(tmp_path, "Y.mtx", N, k, 4)
    args, kw, dt, semiring, Yuse = [fa, "0", "--sddmm", fx, "--out", fo], {}, np.float64, "plus_times", X
    if form != "x_only":
        args += ["--sddmm-y", fy]
        Yuse = Y
    if form == "max_plus":
        args += ["--semiring", "max_plus"]
        semiring = "max_plus"
    elif form == "fp32":
        args += ["--fp32"]
        dt = np.float32
    elif form == "select":
        args += ["--select", "tril:-1"]
        kw["select"] = ("tril", -1)
    elif form == "AAt":
        args = [fr, "0", "1", "--sddmm", fx, "--sddmm-y", fy, "--out", fo]
        kw["aat"] = True
    out = _run(args, _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    assert out.stdout.count("sddmm: ") == 1 and f"k {k}," in out.stdout and "host sum" in out.stdout and "R written to" in out.stdout
    # the pattern is the product's whatever the semiring (section 3g), so the plus_times plan gives it
    I, J = _pattern(pkg, ctx, fr if form == "AAt" else fa, dt, **kw)
    want = sd.sddmm(I, J, X.astype(dt), Yuse.astype(dt), semiring, dt, oracle=oracle)
    gi, gj, gv = _read_coo(fo)
    assert np.array_equal(gi, I) and np.array_equal(gj, J), form
    assert _same(gv, want, dt), form
    row = (tmp_path / "r.csv").read_text().strip().splitlines()[-1].split(",")
    assert len(row) == 22   # (the CSV row describes the product)


def test_sddmm_reaches_the_sorted_coo_files(pkg, oracle, ctx, mats, tmp_path):
    fa, _ = mats
    fx, X = _x(tmp_path, "X.mtx", N, 4, 5)
    out = _run([fa, "1", "--sddmm", fx], _env(tmp_path))
    assert out.returncode == 0 and "sddmm: R = pattern(C) o (X X^T) (plus_times)" in out.stdout and "written" not in out.stdout, out.stdout
    I, J = _pattern(pkg, ctx, fa, np.float64)
    want = sd.sddmm(I, J, X, X, "plus_times", np.float64, oracle=oracle)
    assert int((tmp_path / "SPGEMM_RESULT_NNZ.txt").read_text()) == len(I)
    assert np.array_equal(np.loadtxt(tmp_path / "SPGEMM_RESULT_ROWS.txt", dtype=np.int64), I)
    assert np.array_equal(np.loadtxt(tmp_path / "SPGEMM_RESULT_COLS.txt", dtype=np.int64), J)
    assert (tmp_path / "SPGEMM_RESULT_VALS.txt").read_text().split() == ["%.17f" % v for v in want]


def test_sddmm_refusals(mats, tmp_path):
    fa = mats[0]
    env = _env(tmp_path)
    fx, X = _x(tmp_path, "X.mtx", N, 3, 6)
    fy4, _ = _x(tmp_path, "Y4.mtx", N, 4, 7)
    bad_rows = str(tmp_path / "Xr.mtx")
    _write_array(bad_rows, X[:-1])
    coord = str(tmp_path / "Xc.mtx")
    with open(coord, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n2 2 1\n1 1 1.0\n")
    integer = str(tmp_path / "Xi.mtx")
    _write_array(integer, np.ones((N, 2)), header="%%MatrixMarket matrix array integer general")
    for args, word in (([fa, "0", "--sddmm", fx, "--gpus", "2"], "--gpus"), ([fa, "0", "--sddmm", fx, "--power", "3"], "--power"),
                       ([fa, "0", "--sddmm", fx, "--reduce", "rows"], "--reduce"), ([fa, "0", "--sddmm", fx, "--spmm", fx], "--spmm"),
                       ([fa, "0", "--sddmm-y", fx], "--sddmm-y needs --sddmm"), ([fa, "0", "--sddmm", coord], "not an array"),
                       ([fa, "0", "--sddmm", fx, "--sddmm-y", coord], "not an array"), ([fa, "0", "--sddmm", integer], "not a real"),
                       ([fa, "0", "--sddmm", bad_rows], "X has"), ([fa, "0", "--sddmm", fx, "--sddmm-y", bad_rows], "Y has"),
                       ([fa, "0", "--sddmm", fx, "--sddmm-y", fy4], "columns"), ([fa, "0", "--sddmm", str(tmp_path / "none.mtx")], "cannot open")):
        out = _run(args, env)
        assert out.returncode != 0 and word in out.stdout, (args, out.stdout, out.stderr)
