"""GPU: `pemspgemm A.mtx 0 --extract-rows I.mtx --extract-cols J.mtx [--out C.mtx]` (the final result re-indexed on the device)
against extractref on the golden inputs (tests/golden/spgemm_*.npz; C by the oracle), alone and with --select, --reduce
and --spmm; and its refusals."""
import importlib
import os
import subprocess

import numpy as np
import pytest
import torch

import extractref as ex
import selectref as sel

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("cage4_standin", "rand_300", "rect_70x40_AAt", "powerlaw_600")


def _run(args, env):
    hostio = importlib.import_module("pem_spgemm_amd.hostio")
    return subprocess.run([hostio.CLI_PATH, *args], env=env, capture_output=True, text=True, timeout=120)


def _env(tmp_path):
    return dict(os.environ, PEM_CSV=str(tmp_path / "r.csv"), PEM_REPEAT="2")


def _mtx(path):
    import scipy.io
    C = scipy.io.mmread(path).tocsr()
    C.sort_indices()
    return C


def _golden(standins, oracle, tmp_path, name):
    """(CLI arguments of the product, C's side, C's canonical COO) of a golden input: C = A*A, or A*A^T where the fixture says so, by
    the oracle (the golden C's values come from scipy and agree with it only to rounding; its structure must be the oracle's)"""
    z = np.load(os.path.join(GOLDEN, f"spgemm_{name}.npz"))
    rows, cols, tr = int(z["rows"]), int(z["cols"]), bool(z["transpose"])
    fa = str(tmp_path / f"{name}.mtx")
    standins.write_mtx(fa, rows, cols, z["I"], z["J"], z["V"])
    oa = oracle.Csr(rows, cols, z["I"], z["J"], z["V"])
    ob = oracle.Csr(rows, cols, z["I"], z["J"], z["V"], transpose=True) if tr else oa
    rp, cj, cv = (np.asarray(x) for x in oracle.csr_spgemm(oa, ob).arrays())
    assert np.array_equal(rp, z["c_rowptr"]) and np.array_equal(cj, z["c_colidx"])
    n = rows                                              # A*A (square) or A*A^T: C is rows x rows
    ci = np.repeat(np.arange(n, dtype=np.int32), np.diff(rp))
    return [fa, "0"] + (["1"] if tr else []), n, (ci, cj.astype(np.int32), cv.astype(np.float64))


def _write_list(path, L, field="integer", one_based=True):
    with open(path, "w") as f:
        f.write(f"%%MatrixMarket matrix array {field} general\n% indices\n{len(L)} 1\n")
        for v in L:
            v = int(v) + (1 if one_based else 0)
            f.write(f"{v}\n" if field == "integer" else f"{float(v)!r}\n")
    return path


def _lists(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, n, n + 11), np.concatenate([rng.permutation(n)[: max(1, n // 2)], [n - 1, n - 1]])


def _check(C, shape, I, J, V):
    assert C.shape == shape
    assert np.array_equal(C.indices, J) and np.array_equal(np.diff(C.indptr), np.bincount(I, minlength=shape[0]))
    assert np.array_equal(C.data.view(np.uint8), np.asarray(V, np.float64).view(np.uint8))


@pytest.mark.parametrize("mode", ("rows", "cols", "both"))
@pytest.mark.parametrize("name", NAMES)
def test_extract_matches_extractref_on_the_golden_products(standins, oracle, tmp_path, name, mode):
    args, n, c = _golden(standins, oracle, tmp_path, name)
    RI, CJ = _lists(n, len(name))
    fc = str(tmp_path / "C.mtx")
    if mode != "cols":
        args += ["--extract-rows", _write_list(str(tmp_path / "I.mtx"), RI)]
    if mode != "rows":
        args += ["--extract-cols", _write_list(str(tmp_path / "J.mtx"), CJ, field="real")]
    out = _run(args + ["--out", fc], _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    assert out.stdout.count("extract: ") == 1 and " of C: extract " in out.stdout and "nnz" in out.stdout
    ni, nj, I, J, V = ex.extract(n, n, *c, RI if mode != "cols" else None, CJ if mode != "rows" else None)
    _check(_mtx(fc), (ni, nj), I, J, V)
    assert ", extract " in open(fc).read(400)             # (the comment in the output header)
    row = (tmp_path / "r.csv").read_text().strip().splitlines()[-1].split(",")
    assert len(row) == 22 and int(row[2]) == len(c[0])    # (the CSV row describes the product)


def test_extract_after_select(standins, oracle, tmp_path):
    args, n, c = _golden(standins, oracle, tmp_path, "rand_300")
    RI, CJ = _lists(n, 7)
    fc = str(tmp_path / "C.mtx")
    out = _run(args + ["--extract-rows", _write_list(str(tmp_path / "I.mtx"), RI), "--extract-cols", _write_list(str(tmp_path / "J.mtx"), CJ),
                       "--select", "abs_gt:0.3", "--out", fc], _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    assert out.stdout.index("select: ") < out.stdout.index("extract: ") and "of the selection" in out.stdout
    s = sel.select(*c, "abs_gt", 0.3)
    ni, nj, I, J, V = ex.extract(n, n, *s, RI, CJ)
    _check(_mtx(fc), (ni, nj), I, J, V)


def _read_array(path):
    lines = [ln for ln in open(path).read().splitlines() if not ln.startswith("%")]
    r, k = (int(x) for x in lines[0].split())
    v = np.array([float(x) for x in lines[1:]], np.float64)
    assert len(v) == r * k
    return v.reshape(k, r).T


def _same(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return got.shape == want.shape and bool(np.all(got.view(np.uint64) == want.view(np.uint64)))


@pytest.mark.parametrize("dim", ("rows", "cols"))
def test_reduce_sees_the_extract(pkg, ctx, standins, oracle, tmp_path, dim):
    args, n, c = _golden(standins, oracle, tmp_path, "powerlaw_600")
    RI, CJ = _lists(n, 3)
    fv = str(tmp_path / "v.mtx")
    out = _run(args + ["--extract-rows", _write_list(str(tmp_path / "I.mtx"), RI), "--extract-cols", _write_list(str(tmp_path / "J.mtx"), CJ),
                       "--reduce", dim, "--out", fv], _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    assert "of the extract" in out.stdout
    ni, nj, I, J, V = ex.extract(n, n, *c, RI, CJ)
    want = pkg.Tiled.from_coo(ctx, ni, nj, I, J, V).reduce("plus", dim)
    ctx.synchronize()
    got = _read_array(fv)
    assert got.shape == ((ni if dim == "rows" else nj), 1) and _same(got[:, 0], want.cpu().numpy())


def test_spmm_sees_the_extract_and_checks_its_shape(pkg, ctx, standins, oracle, tmp_path):
    args, n, c = _golden(standins, oracle, tmp_path, "rect_70x40_AAt")
    RI, CJ = _lists(n, 5)
    ni, nj, I, J, V = ex.extract(n, n, *c, RI, CJ)
    X = np.random.default_rng(2).uniform(-2, 2, (nj, 3))
    fx, fy = str(tmp_path / "X.mtx"), str(tmp_path / "Y.mtx")
    with open(fx, "w") as f:
        f.write(f"%%MatrixMarket matrix array real general\n{nj} 3\n")
        for v in X.T.ravel():
            f.write(f"{float(v)!r}\n")
    lists = ["--extract-rows", _write_list(str(tmp_path / "I.mtx"), RI), "--extract-cols", _write_list(str(tmp_path / "J.mtx"), CJ)]
    out = _run(args + lists + ["--spmm", fx, "--out", fy], _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    assert "spmm: Y = the extract" in out.stdout
    Y = pkg.Tiled.from_coo(ctx, ni, nj, I, J, V).spmm(torch.from_numpy(np.ascontiguousarray(X)).cuda())
    ctx.synchronize()
    assert _same(_read_array(fy), Y.cpu().numpy())
    out = _run(args + lists[:2] + ["--spmm", fx], _env(tmp_path))   # without the column list the result has n columns, X has nj rows
    assert out.returncode == 1 and "rows; the result has" in out.stdout, out.stdout


def test_extract_refusals(standins, oracle, tmp_path):
    args, n, _ = _golden(standins, oracle, tmp_path, "rand_300")
    env = _env(tmp_path)
    good = _write_list(str(tmp_path / "I.mtx"), [0, 5, 5])

    def text(name, body):
        p = str(tmp_path / name)
        with open(p, "w") as f:
            f.write(body)
        return p

    hdr = "%%MatrixMarket matrix array integer general\n"
    cases = ((["--extract-rows", good, "--gpus", "2"], "--gpus"), (["--extract-cols", good, "--gpus", "2"], "--gpus"),
             (["--extract-rows", str(tmp_path / "none.mtx")], "cannot open"),
             (["--extract-rows", text("coord.mtx", "%%MatrixMarket matrix coordinate real general\n2 2 1\n1 1 1.0\n")], "not an array"),
             (["--extract-cols", text("cplx.mtx", "%%MatrixMarket matrix array complex general\n1 1\n1 0\n")], "not an integer or real"),
             (["--extract-rows", text("two.mtx", hdr + "2 2\n1\n2\n3\n4\n")], "columns"),
             (["--extract-rows", text("short.mtx", hdr + "3 1\n1\n2\n")], "fewer values"),
             (["--extract-rows", text("nosize.mtx", hdr)], "no size line"),
             (["--extract-rows", text("empty.mtx", hdr + "0 1\n")], "indices"),
             (["--extract-rows", text("frac.mtx", "%%MatrixMarket matrix array real general\n2 1\n1.0\n2.5\n")], "not an integer"),
             (["--extract-rows", text("zero.mtx", hdr + "2 1\n1\n0\n")], "out of range"),
             (["--extract-cols", text("neg.mtx", hdr + "1 1\n-4\n")], "out of range"),
             (["--extract-rows", text("big.mtx", hdr + f"2 1\n1\n{n + 1}\n")], f"the result has {n} rows"),
             (["--extract-cols", text("bigc.mtx", hdr + f"1 1\n{n + 1}\n")], f"the result has {n} columns"))
    for extra, word in cases:
        out = _run(args + extra, env)
        assert out.returncode == 1 and word in out.stdout, (extra, out.stdout, out.stderr)
