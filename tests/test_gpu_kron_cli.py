"""GPU: `pemspgemm A.mtx 0 --kron K.mtx [--kron-op OP] [--out R.mtx]` (the final result becomes (result) (x) K on the device) against
kronref of the oracle's A*A with K, alone, with --kron-op plus, with --fp32, followed by --reduce rows and by --bfs 1; and the new
refusals."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import frontierref
import kronref

pytestmark = pytest.mark.gpu

N = 60
KR, KC = 5, 7


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


@pytest.fixture
def mats(standins, oracle, tmp_path):
    rng = np.random.default_rng(53)
    fa, fk, fs = str(tmp_path / "A.mtx"), str(tmp_path / "K.mtx"), str(tmp_path / "S.mtx")
    A, K, S = _rand(rng, N, N, 400), _rand(rng, KR, KC, 17), _rand(rng, 4, 4, 9)
    standins.write_mtx(fa, N, N, *A)
    standins.write_mtx(fk, KR, KC, *K)
    standins.write_mtx(fs, 4, 4, *S)                             # a square K: the product stays square for --bfs
    return dict(A=fa, K=fk, S=fs, a=A, k=K, s=S)


def _product(oracle, mats, dt):
    """the oracle's A*A in the value type: (I, J, V)"""
    I, J, V = mats["a"]
    a = oracle.Csr(N, N, I, J, np.asarray(V, dt).astype(np.float64))
    rp, ci, v = oracle.csr_spgemm(a, a, f32=dt == np.float32).arrays()
    return np.repeat(np.arange(N, dtype=np.int32), np.diff(rp)), np.asarray(ci, np.int32), np.asarray(v).astype(dt)


def _same(path, want, dt):
    rows, cols, I, J, V = want
    gI, gJ, gV, shape = _coo(path)
    assert shape == (rows, cols)
    assert np.array_equal(gI, I) and np.array_equal(gJ, J)
    assert np.array_equal(gV.astype(dt).view(np.uint8), np.asarray(V, dt).view(np.uint8))


@pytest.mark.parametrize("fp32", (False, True), ids=("f64", "f32"))
@pytest.mark.parametrize("op", ("times", "plus"))
def test_kron_matches_kronref_of_the_oracles_product(mats, oracle, tmp_path, op, fp32):
    dt = np.float32 if fp32 else np.float64
    fc = str(tmp_path / "R.mtx")
    flags = (["--kron-op", op] if op != "times" else []) + (["--fp32"] if fp32 else [])
    out = _run([mats["A"], "0", "--kron", mats["K"], "--out", fc] + flags, _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    assert out.stdout.count(f"kron: C (x) {mats['K']} under {op}") == 1
    kI, kJ, kV = mats["k"]
    want = kronref.kron(N, N, *_product(oracle, mats, dt), KR, KC, kI, kJ, np.asarray(kV, dt), op, dt)
    assert f"{N * KR} x {N * KC}, nnz {len(want[2])}" in out.stdout
    _same(fc, want, dt)
    row = (tmp_path / "r.csv").read_text().strip().splitlines()[-1].split(",")
    assert len(row) == 22                                        # (the CSV row describes the product)


def test_kron_then_reduce_rows(mats, oracle, tmp_path):
    fc = str(tmp_path / "y.mtx")
    out = _run([mats["A"], "0", "--kron", mats["K"], "--reduce", "rows", "--out", fc], _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    assert "reduce: rows plus of the Kronecker product" in out.stdout
    kI, kJ, kV = mats["k"]
    rows, cols, I, J, V = kronref.kron(N, N, *_product(oracle, mats, np.float64), KR, KC, kI, kJ, kV, "times", np.float64)
    want = np.zeros(rows)
    for i, v in zip(I, V):                                       # the fold of every row's entries in ascending column order, from 0
        want[i] += v
    import scipy.io
    got = np.asarray(scipy.io.mmread(fc)).ravel()
    assert got.shape == (rows,) and np.array_equal(got, want)


def test_kron_then_bfs(mats, oracle, tmp_path):
    fc = str(tmp_path / "levels.mtx")
    out = _run([mats["A"], "0", "--kron", mats["S"], "--bfs", "1", "--out", fc], _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    sI, sJ, sV = mats["s"]
    rows, cols, I, J, V = kronref.kron(N, N, *_product(oracle, mats, np.float64), 4, 4, sI, sJ, sV, "times", np.float64)
    rp = np.concatenate([[0], np.cumsum(np.bincount(I, minlength=rows))]).astype(np.int64)
    want, depth, reached = frontierref.bfs(rows, rp, J.astype(np.int64), 0)
    assert f"bfs: from 1 over the Kronecker product: depth {depth}, reached {reached} of {rows}" in out.stdout
    import scipy.io
    got = np.asarray(scipy.io.mmread(fc)).ravel()
    assert np.array_equal(got.astype(np.int64), want.astype(np.int64))


def test_overflow_prints_the_librarys_message(standins, tmp_path):
    """a 40 000 x 40 000 product with a 60 000 x 60 000 K: 2 400 000 000 rows"""
    fa, fk, fc = str(tmp_path / "A.mtx"), str(tmp_path / "K.mtx"), str(tmp_path / "R.mtx")
    standins.write_mtx(fa, 40_000, 40_000, np.array([5, 7], np.int32), np.array([7, 9], np.int32), np.array([1.0, 2.0]))
    standins.write_mtx(fk, 60_000, 60_000, np.array([1], np.int32), np.array([2], np.int32), np.array([3.0]))
    out = _run([fa, "0", "--kron", fk, "--out", fc], _env(tmp_path))
    assert out.returncode == 1, out.stdout + out.stderr
    lines = [l for l in out.stdout.splitlines() if l.startswith("--kron")]
    assert len(lines) == 1 and "pem_tiled_kron: the result would be 2400000000 x 2400000000" in lines[0] and lines[0].endswith("Exiting.")
    assert not os.path.exists(fc)


REFUSALS = (
    (["--kron-op", "plus"], "--kron-op needs --kron <K.mtx>. Exiting."),
    (["--kron", "{K}", "--gpus", "2"], "--kron does not combine with --gpus. Exiting."),
    (["--kron", "{K}", "--kron-op", "minus"], "--kron-op minus: unknown op (plus, times, min, max, lor, land). Exiting."),
)


@pytest.mark.parametrize("k", range(len(REFUSALS)))
def test_new_refusals_print_one_line_and_exit_1(mats, tmp_path, k):
    args, line = REFUSALS[k]
    fc = str(tmp_path / "R.mtx")
    out = _run([mats["A"], "0", *[a.format(K=mats["K"]) for a in args], "--out", fc], _env(tmp_path))
    assert out.returncode == 1, out.stdout + out.stderr
    assert out.stdout.strip().splitlines() == [line]
    assert not os.path.exists(fc)
