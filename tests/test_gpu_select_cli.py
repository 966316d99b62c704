"""GPU: `pemspgemm A.mtx 0 --select OP[:THUNK] [--out C.mtx]` (the final result filtered on the device) against the oracle's product
filtered by scipy / selectref, alone and with --semiring, --mask, --add and --fp32; and its refusals."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import ewiseref as er
import selectref as sel
import semiringref as sr

pytestmark = pytest.mark.gpu

N = 150


def _rand(rng, r, c, nz):
    key = np.sort(rng.choice(r * c, nz, replace=False))
    return (key // c).astype(np.int32), (key % c).astype(np.int32), rng.uniform(-1, 1, nz)


def _run(args, env):
    hostio = importlib.import_module("pem_spgemm_amd.hostio")
    return subprocess.run([hostio.CLI_PATH, *args], env=env, capture_output=True, text=True, timeout=120)


def _env(tmp_path, name="r.csv"):
    return dict(os.environ, PEM_CSV=str(tmp_path / name), PEM_REPEAT="2")


def _mtx(path):
    import scipy.io
    C = scipy.io.mmread(path).tocsr()
    C.sort_indices()
    return C


def _coo_of(rp, ci, v):
    return np.repeat(np.arange(len(rp) - 1, dtype=np.int32), np.diff(rp)), np.asarray(ci, np.int32), np.asarray(v)


@pytest.fixture
def mats(standins, tmp_path):
    rng = np.random.default_rng(43)
    a, d, m = _rand(rng, N, N, 1200), _rand(rng, N, N, 2000), _rand(rng, N, N, 6000)
    fa, fd, fm = str(tmp_path / "A.mtx"), str(tmp_path / "D.mtx"), str(tmp_path / "M.mtx")
    standins.write_mtx(fa, N, N, *a)
    standins.write_mtx(fd, N, N, *d)
    standins.write_mtx(fm, N, N, *m)
    return fa, fd, fm, a, d, m


def _check(C, I, J, V, dt):
    assert np.array_equal(C.indices, J) and np.array_equal(np.diff(C.indptr), np.bincount(I, minlength=N))
    assert np.array_equal(C.data.astype(dt).view(np.uint8), np.asarray(V, dt).view(np.uint8))


@pytest.mark.parametrize("fp32", (False, True), ids=("f64", "f32"))
@pytest.mark.parametrize("spec", ("abs_gt:0.05", "tril:-1", "value_ne:0", "triu", "diag:3", "value_lt:-0.1", "col_gt:70"))
def test_select_matches_filtered_oracle(mats, oracle, tmp_path, spec, fp32):
    fa, a = mats[0], mats[3]
    fc = str(tmp_path / "C.mtx")
    out = _run([fa, "0", "--select", spec, "--out", fc] + (["--fp32"] if fp32 else []), _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    assert out.stdout.count("select: ") == 1 and " kept" in out.stdout
    dt = np.float32 if fp32 else np.float64
    oa = oracle.Csr(N, N, a[0], a[1], a[2].astype(dt).astype(np.float64))
    c = _coo_of(*oracle.csr_spgemm(oa, oa, f32=fp32).arrays())
    op, _, th = spec.partition(":")
    I, J, V = sel.select(c[0], c[1], c[2], op, float(th) if th else 0, dt)
    _check(_mtx(fc), I, J, V, dt)
    row = (tmp_path / "r.csv").read_text().strip().splitlines()[-1].split(",")
    assert len(row) == 22 and int(row[2]) == len(c[0])   # (the CSV row describes the product)


def test_select_matches_scipy(mats, tmp_path):
    import scipy.sparse as sp
    fa, a = mats[0], mats[3]
    fc = str(tmp_path / "C.mtx")
    out = _run([fa, "0", "--select", "abs_gt:0.2", "--out", fc], _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    A = sp.csr_matrix((a[2], (a[0], a[1])), shape=(N, N))
    S = (A @ A).tocoo()
    keep = np.abs(S.data) > 0.2
    S = sp.csr_matrix((S.data[keep], (S.row[keep], S.col[keep])), shape=(N, N))
    S.sort_indices()
    C = _mtx(fc)
    assert np.array_equal(S.indptr, C.indptr) and np.array_equal(S.indices, C.indices)
    assert np.allclose(S.data, C.data, rtol=1e-12, atol=1e-12)


def test_select_with_semiring(mats, tmp_path):
    fa, a = mats[0], mats[3]
    fc = str(tmp_path / "C.mtx")
    out = _run([fa, "0", "--semiring", "min_plus", "--select", "value_lt:-0.5", "--out", fc], _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    ac = sr.coo_to_csr(N, N, *a)
    c = _coo_of(*sr.spgemm(ac, ac, N, "min_plus"))
    _check(_mtx(fc), *sel.select(*c, "value_lt", -0.5), np.float64)


@pytest.mark.parametrize("complement", (False, True), ids=("mask", "complement"))
def test_select_with_mask(mats, oracle, tmp_path, complement):
    fa, fm, a, m = mats[0], mats[2], mats[3], mats[5]
    fc = str(tmp_path / "C.mtx")
    out = _run([fa, "0", "--mask", fm] + (["--mask-complement"] if complement else []) + ["--select", "tril:2", "--out", fc], _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    oa = oracle.Csr(N, N, *a)
    c = _coo_of(*oracle.csr_spgemm(oa, oa).arrays())
    inm = np.isin(c[0].astype(np.int64) * N + c[1], m[0].astype(np.int64) * N + m[1])
    keep = ~inm if complement else inm
    _check(_mtx(fc), *sel.select(c[0][keep], c[1][keep], c[2][keep], "tril", 2), np.float64)


@pytest.mark.parametrize("fp32", (False, True), ids=("f64", "f32"))
def test_select_with_add(mats, oracle, tmp_path, fp32):
    fa, fd, a, d = mats[0], mats[1], mats[3], mats[4]
    fc = str(tmp_path / "C.mtx")
    out = _run([fa, "0", "--add", fd, "--alpha", "2", "--beta", "-0.5", "--select", "abs_gt:0.3", "--out", fc] + (["--fp32"] if fp32 else []),
               _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    assert "select: abs_gt:0.3 of the sum" in out.stdout
    dt = np.float32 if fp32 else np.float64
    oa = oracle.Csr(N, N, a[0], a[1], a[2].astype(dt).astype(np.float64))
    c = _coo_of(*oracle.csr_spgemm(oa, oa, f32=fp32).arrays())
    s = er.ewise(N, (c[0], c[1], c[2].astype(dt)), (d[0], d[1], d[2].astype(dt)), "plus", "union", 2.0, -0.5)
    _check(_mtx(fc), *sel.select(*s, "abs_gt", 0.3, dt), dt)


def test_select_refusals(mats, tmp_path):
    fa = mats[0]
    env = _env(tmp_path)
    for args, word in (([fa, "0", "--select", "tril", "--gpus", "2"], "--gpus"), ([fa, "0", "--select", "tril", "--power", "3"], "--power"),
                       ([fa, "0", "--select", "lower:0"], "unknown op"), ([fa, "0", "--select", "abs_gt:1e-x"], "does not parse"),
                       ([fa, "0", "--select", "abs_gt:"], "does not parse"), ([fa, "0", "--select", "tril:0.5"], "integral"),
                       ([fa, "0", "--select", "diag:nan"], "integral"), ([fa, "0", "--select", "row_le:1e12"], "integral")):
        out = _run(args, env)
        assert out.returncode != 0 and word in out.stdout, (args, out.stdout, out.stderr)
    assert not os.path.exists(tmp_path / "r.csv")
