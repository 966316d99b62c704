"""GPU: `pemspgemm A.mtx 0 --spmm X.mtx [--out Y.mtx]` (Y = R (+).(x) X on the device, R the final result) against Tiled.spmm of the
same R built through the Python binding -- alone and with --add, --select, --semiring min_plus, --fp32 and A*A^T; and its refusals."""
import importlib
import os
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

torch.cuda.is_available()

N, M = 150, 110   # A is N x M: A*A^T is N x N, A^2 needs a square A


def _rand(rng, r, c, nz):
    key = np.sort(rng.choice(r * c, nz, replace=False))
    return (key // c).astype(np.int32), (key % c).astype(np.int32), rng.uniform(-1, 1, nz)


def _run(args, env):
    hostio = importlib.import_module("pem_spgemm_amd.hostio")
    return subprocess.run([hostio.CLI_PATH, *args], env=env, capture_output=True, text=True, timeout=120)


def _env(tmp_path):
    return dict(os.environ, PEM_CSV=str(tmp_path / "r.csv"), PEM_REPEAT="2")


def _read_coo(path):
    import scipy.io
    A = scipy.io.mmread(path).tocoo()
    return A.row.astype(np.int32), A.col.astype(np.int32), A.data.astype(np.float64)


def _write_array(path, X, header="%%MatrixMarket matrix array real general"):
    with open(path, "w") as f:
        f.write(f"{header}\n% X\n{X.shape[0]} {X.shape[1]}\n")
        for v in X.T.ravel():   # column by column
            f.write(f"{float(v)!r}\n")


def _read_array(path):
    lines = [ln for ln in open(path).read().splitlines() if not ln.startswith("%")]
    r, k = (int(x) for x in lines[0].split())
    v = np.array([float(x) for x in lines[1:]], np.float64)
    assert len(v) == r * k
    return v.reshape(k, r).T


@pytest.fixture
def mats(standins, tmp_path):
    rng = np.random.default_rng(53)
    a, d, r = _rand(rng, N, N, 1500), _rand(rng, N, N, 2000), _rand(rng, N, M, 1300)
    keep = (a[0] % 17 != 3) & (a[1] % 13 != 5)   # some empty rows and columns
    a = tuple(x[keep] for x in a)
    fa, fd, fr = str(tmp_path / "A.mtx"), str(tmp_path / "D.mtx"), str(tmp_path / "R.mtx")
    standins.write_mtx(fa, N, N, *a)
    standins.write_mtx(fd, N, N, *d)
    standins.write_mtx(fr, N, M, *r)
    return fa, fd, fr


def _x(tmp_path, n, k, seed=3):
    # values exact in fp32, so the fp64 and fp32 runs read the same numbers
    X = np.random.default_rng(seed).uniform(-2, 2, (n, k)).astype(np.float32).astype(np.float64)
    X[::7, 0] = 0.0
    fx = str(tmp_path / "X.mtx")
    _write_array(fx, X)
    return fx, X


def _expected(pkg, ctx, fa, fd, X, dtype, semiring, aat=False, add=None, select=None):
    rows, cols = (N, M) if aat else (N, N)
    A = pkg.Tiled.from_coo(ctx, rows, cols, *_read_coo(fa), dtype=dtype)
    if aat:
        At = pkg.Tiled.from_coo(ctx, rows, cols, *_read_coo(fa), transpose=True, dtype=dtype)
        p = pkg.CPlan(ctx, A, At, semiring=semiring)
    else:
        p = pkg.CPlan(ctx, A, A, semiring=semiring)
    p.spgemm()
    R = pkg.Tiled.from_cplan(p)
    if add is not None:
        D = pkg.Tiled.from_coo(ctx, N, N, *_read_coo(fd), dtype=dtype)
        R = pkg.Tiled.ewise(R, D, "plus", "union", 1.0, 1.0)
    if select is not None:
        R = R.select(*select)
    Y = R.spmm(torch.from_numpy(np.ascontiguousarray(X.astype(dtype))).cuda(), semiring)
    torch.cuda.synchronize()
    ctx.synchronize()
    return Y.cpu().numpy().astype(np.float64)


def _same(got, want, dtype=np.float64):
    """bit equality in the value type (the CLI writes fp32 values with 9 significant digits: they read back exactly as floats)"""
    got, want = np.asarray(got).astype(dtype), np.asarray(want).astype(dtype)
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    return got.shape == want.shape and bool(np.all((got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want))))


@pytest.mark.parametrize("form", ("plain", "add", "select", "min_plus", "fp32", "AAt"))
def test_spmm_matches_tiled_spmm(pkg, ctx, mats, tmp_path, form):
    fa, fd, fr = mats
    fy = str(tmp_path / "Y.mtx")
    k = 5
    fx, X = _x(tmp_path, N, k)
    args, kw, dt = [fa, "0", "--spmm", fx, "--out", fy], {}, np.float64
    if form == "add":
        args += ["--add", fd]
        kw["add"] = True
    elif form == "select":
        args += ["--select", "abs_gt:0.3"]
        kw["select"] = ("abs_gt", 0.3)
    elif form == "min_plus":
        args += ["--semiring", "min_plus"]
    elif form == "fp32":
        args += ["--fp32"]
        dt = np.float32
    elif form == "AAt":
        args = [fr, "0", "1", "--spmm", fx, "--out", fy]
        kw["aat"] = True
    out = _run(args, _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    assert out.stdout.count("spmm: ") == 1 and f"k {k}," in out.stdout and "host sum" in out.stdout and "Y written to" in out.stdout
    semiring = "min_plus" if form == "min_plus" else "plus_times"
    want = _expected(pkg, ctx, fr if form == "AAt" else fa, fd, X, dt, semiring, **kw)
    assert _same(_read_array(fy), want, dt), form
    row = (tmp_path / "r.csv").read_text().strip().splitlines()[-1].split(",")
    assert len(row) == 22   # (the CSV row describes the product)


def test_spmm_without_out_prints_only(mats, tmp_path):
    fx, _ = _x(tmp_path, N, 3)
    out = _run([mats[0], "0", "--spmm", fx], _env(tmp_path))
    assert out.returncode == 0 and "spmm: Y = C (plus_times) X" in out.stdout and "written" not in out.stdout, out.stdout


def test_spmm_refusals(mats, tmp_path):
    fa = mats[0]
    env = _env(tmp_path)
    fx, X = _x(tmp_path, N, 3)
    bad_rows = str(tmp_path / "Xr.mtx")
    _write_array(bad_rows, X[:-1])
    coord = str(tmp_path / "Xc.mtx")
    with open(coord, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n2 2 1\n1 1 1.0\n")
    integer = str(tmp_path / "Xi.mtx")
    _write_array(integer, np.ones((N, 2)), header="%%MatrixMarket matrix array integer general")
    cplx = str(tmp_path / "Xz.mtx")
    _write_array(cplx, np.ones((N, 2)), header="%%MatrixMarket matrix array complex general")
    for args, word in (([fa, "0", "--spmm", fx, "--gpus", "2"], "--gpus"), ([fa, "0", "--spmm", fx, "--power", "3"], "--power"),
                       ([fa, "0", "--spmm", fx, "--reduce", "rows"], "--reduce"), ([fa, "0", "--spmm", coord], "not an array"),
                       ([fa, "0", "--spmm", integer], "not a real"), ([fa, "0", "--spmm", cplx], "not a real"),
                       ([fa, "0", "--spmm", bad_rows], "rows"), ([fa, "0", "--spmm", str(tmp_path / "none.mtx")], "cannot open")):
        out = _run(args, env)
        assert out.returncode != 0 and word in out.stdout, (args, out.stdout, out.stderr)


def test_matrix_reader_still_refuses_arrays(pkg, tmp_path):
    """pem_mm_read keeps refusing array files: X is read by the CLI's own parser"""
    hostio = importlib.import_module("pem_spgemm_amd.hostio")
    fx, _ = _x(tmp_path, 4, 2)
    with pytest.raises(Exception):
        hostio.mm_read(fx)
