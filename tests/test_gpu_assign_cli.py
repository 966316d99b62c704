"""GPU: `pemspgemm A.mtx S --assign-into D.mtx [--assign-rows I.mtx] [--assign-cols J.mtx] [--assign-accum OP]` (the final result
written into D on the device) against assignref on matrices written in the test (C by the oracle): --out, the sorted COO files, the
CSV row; and its refusals."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import assignref as ar
import extractref as ex
from test_gpu_extract_cli import _check, _mtx, _write_list

pytestmark = pytest.mark.gpu

N, DR, DC = 60, 90, 80                                    # A is N x N; D is DR x DC


def _run(args, env):
    hostio = importlib.import_module("pem_spgemm_amd.hostio")
    return subprocess.run([hostio.CLI_PATH, *args], env=env, capture_output=True, text=True, timeout=120)


def _env(tmp_path):
    return dict(os.environ, PEM_CSV=str(tmp_path / "r.csv"), PEM_REPEAT="2", PEM_RESULT_DIR=str(tmp_path))


def _coo(rng, rows, cols, nnz):
    key = np.sort(rng.choice(rows * cols, nnz, replace=False))
    return (key // cols).astype(np.int32), (key % cols).astype(np.int32), rng.uniform(-2, 2, nnz)


@pytest.fixture()
def inputs(standins, oracle, tmp_path):
    """A.mtx and C = A*A by the oracle (canonical COO); D.mtx (DR x DC) and a D of C's shape; the lists"""
    rng = np.random.default_rng(5)
    a = _coo(rng, N, N, 400)
    fa = str(tmp_path / "A.mtx")
    standins.write_mtx(fa, N, N, *a)
    oa = oracle.Csr(N, N, *a)
    rp, cj, cv = (np.asarray(x) for x in oracle.csr_spgemm(oa, oa).arrays())
    c = (np.repeat(np.arange(N, dtype=np.int32), np.diff(rp)), cj.astype(np.int32), cv.astype(np.float64))
    d, dn = _coo(rng, DR, DC, 1500), _coo(rng, N, N, 700)
    fd, fdn = str(tmp_path / "D.mtx"), str(tmp_path / "Dn.mtx")
    standins.write_mtx(fd, DR, DC, *d)
    standins.write_mtx(fdn, N, N, *dn)
    RI, CJ = rng.permutation(DR)[:N], rng.permutation(DC)[:N]
    return dict(fa=fa, c=c, d=d, fd=fd, dn=dn, fdn=fdn, RI=RI, CJ=CJ, fi=_write_list(str(tmp_path / "I.mtx"), RI),
                fj=_write_list(str(tmp_path / "J.mtx"), CJ, field="real"))


def _check_coo_files(tmp_path, I, J, V):
    assert int((tmp_path / "SPGEMM_RESULT_NNZ.txt").read_text()) == len(I)
    assert np.array_equal(np.loadtxt(tmp_path / "SPGEMM_RESULT_ROWS.txt", dtype=np.int64, ndmin=1), I)
    assert np.array_equal(np.loadtxt(tmp_path / "SPGEMM_RESULT_COLS.txt", dtype=np.int64, ndmin=1), J)
    assert (tmp_path / "SPGEMM_RESULT_VALS.txt").read_text().splitlines() == ["%.17f" % v for v in V]


@pytest.mark.parametrize("accum", (None, "plus", "min"))
def test_assign_rows_and_cols(inputs, tmp_path, accum):
    z = inputs
    fc = str(tmp_path / "Z.mtx")
    out = _run([z["fa"], "1", "--assign-into", z["fd"], "--assign-rows", z["fi"], "--assign-cols", z["fj"], "--out", fc]
               + (["--assign-accum", accum] if accum else []), _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    assert out.stdout.count("assign: ") == 1 and "assign: C into " in out.stdout and "nnz" in out.stdout
    assert (", accum " + accum in out.stdout) if accum else (", accum " not in out.stdout)
    I, J, V = ar.assign(DR, DC, z["d"], z["c"], z["RI"], z["CJ"], accum)
    _check(_mtx(fc), (DR, DC), I, J, V)
    assert ", assigned into " in open(fc).read(400)       # (the comment in the output header)
    _check_coo_files(tmp_path, I, J, V)
    row = (tmp_path / "r.csv").read_text().strip().splitlines()[-1].split(",")
    assert len(row) == 22 and int(row[2]) == len(z["c"][0])   # (the CSV row describes the product)


def test_assign_without_lists_and_after_select_and_extract(inputs, tmp_path):
    z = inputs
    fc = str(tmp_path / "Z.mtx")
    out = _run([z["fa"], "0", "--assign-into", z["fdn"], "--assign-accum", "max", "--out", fc], _env(tmp_path))   # all rows, all columns
    assert out.returncode == 0, out.stderr + out.stdout
    assert "all rows x all columns" in out.stdout
    _check(_mtx(fc), (N, N), *ar.assign(N, N, z["dn"], z["c"], None, None, "max"))
    # the extract of C (20 rows, all columns) into 20 rows of Dn
    XI, AI = np.arange(5, 25), np.arange(N)[::-3]
    out = _run([z["fa"], "0", "--extract-rows", _write_list(str(tmp_path / "XI.mtx"), XI), "--assign-into", z["fdn"], "--assign-rows",
                _write_list(str(tmp_path / "AI.mtx"), AI), "--out", fc], _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    assert out.stdout.index("extract: ") < out.stdout.index("assign: ") and "assign: the extract into " in out.stdout
    ni, nj, ei, ej, ev = ex.extract(N, N, *z["c"], XI, None)
    _check(_mtx(fc), (N, N), *ar.assign(N, N, z["dn"], (ei, ej, ev), AI, None, None))
    head = open(fc).read(400)
    assert ", extract " in head and ", assigned into " in head


def test_assign_refusals(inputs, tmp_path):
    z = inputs
    env = _env(tmp_path)
    args = [z["fa"], "0"]
    hdr = "%%MatrixMarket matrix array integer general\n"

    def text(name, body):
        p = str(tmp_path / name)
        with open(p, "w") as f:
            f.write(body)
        return p

    into = ["--assign-into", z["fd"], "--assign-rows", z["fi"], "--assign-cols", z["fj"]]
    cases = ((["--assign-rows", z["fi"]], "--assign-rows needs --assign-into"), (["--assign-cols", z["fj"]], "--assign-cols needs --assign-into"),
             (["--assign-accum", "plus"], "--assign-accum needs --assign-into"),
             (into + ["--gpus", "2"], "--gpus"), (into + ["--power", "2"], "--power"),
             (into + ["--assign-accum", "second"], "unknown op"),
             (["--assign-into", z["fd"], "--assign-rows", str(tmp_path / "none.mtx")], "cannot open"),
             (["--assign-into", z["fd"], "--assign-cols", z["fj"], "--assign-rows", text("rep.mtx", hdr + "3 1\n4\n9\n4\n")], "is repeated"),
             (["--assign-into", z["fd"], "--assign-rows", z["fi"], "--assign-cols", text("zero.mtx", hdr + "2 1\n1\n0\n")], "out of range"),
             (["--assign-into", z["fd"], "--assign-cols", z["fj"], "--assign-rows", text("big.mtx", hdr + f"2 1\n1\n{DR + 1}\n")], f"has {DR} rows"),
             (["--assign-into", z["fd"], "--assign-rows", z["fi"], "--assign-cols", text("bigc.mtx", hdr + f"1 1\n{DC + 1}\n")], f"has {DC} columns"),
             (["--assign-into", z["fd"]], f"the result is {N} x {N} but the region is {DR} x {DC}"),
             (["--assign-into", z["fd"], "--assign-rows", z["fi"]], f"the region is {N} x {DC}"),
             (into[:4] + ["--assign-cols", _write_list(str(tmp_path / "J3.mtx"), [0, 1, 2])], f"the region is {N} x 3"))
    for extra, word in cases:
        out = _run(args + extra, env)
        assert out.returncode == 1 and word in out.stdout, (extra, out.stdout, out.stderr)
