"""GPU: `pemspgemm A.mtx 0 --sampled S.mtx [--sampled-bt] [--B B.mtx] --out R.mtx` (the sampled product of the two operands at S's
pattern, in place of the plan product) against sampledref, with --semiring, --fp32 and the A*A^T argument; `--triangles` against
the numpy count; the shape refusals, which need the operands; and a default run, which the new flags leave as it was."""
import importlib
import os
import subprocess

import numpy as np
import pytest
import torch

import sampledref as sr

pytestmark = pytest.mark.gpu

torch.cuda.is_available()

N, M, P = 150, 110, 90   # A is N x M; B is M x P, or P x M for --sampled-bt; S is N x P


def _rand(rng, r, c, nz):
    key = np.sort(rng.choice(r * c, nz, replace=False))
    # values exact in fp32, so the fp64 and fp32 runs read the same numbers
    return (key // c).astype(np.int32), (key % c).astype(np.int32), rng.uniform(-1, 1, nz).astype(np.float32).astype(np.float64)


def _run(args, env):
    hostio = importlib.import_module("pem_spgemm_amd.hostio")
    return subprocess.run([hostio.CLI_PATH, *args], env=env, capture_output=True, text=True, timeout=120)


def _env(tmp_path):
    return dict(os.environ, PEM_CSV=str(tmp_path / "r.csv"), PEM_REPEAT="2", PEM_RESULT_DIR=str(tmp_path))


def _read_coo(path):
    """a coordinate file as written by the CLI (inf and nan values included, which a start value may be)"""
    with open(path) as f:
        lines = [l.split() for l in f if not l.startswith("%")]
    rows = lines[1:]
    assert int(lines[0][2]) == len(rows)
    return (np.array([int(r[0]) - 1 for r in rows], np.int32), np.array([int(r[1]) - 1 for r in rows], np.int32),
            np.array([float(r[2]) for r in rows], np.float64))


def _same(got, want, dtype):
    got, want = np.asarray(got).astype(dtype), np.asarray(want).astype(dtype)
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    return got.shape == want.shape and bool(np.all((got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want))))


@pytest.fixture
def mats(standins, tmp_path):
    rng = np.random.default_rng(61)
    m = dict(A=(N, M, _rand(rng, N, M, 1400)), B=(M, P, _rand(rng, M, P, 1200)), S=(N, P, _rand(rng, N, P, 900)), SA=(N, N, _rand(rng, N, N, 1000)))
    m["Bt"] = (P, M, (m["B"][2][1], m["B"][2][0], m["B"][2][2]))
    files = {}
    for k, (r, c, (i, j, v)) in m.items():
        files[k] = str(tmp_path / f"{k}.mtx")
        o = np.lexsort((j, i))
        standins.write_mtx(files[k], r, c, i[o], j[o], v[o])
    return m, files


@pytest.mark.parametrize("form", ("plain", "bt", "max_plus", "fp32", "AAt", "plus_pair_bt"))
def test_sampled_matches_the_reference(oracle, mats, tmp_path, form):
    m, f = mats
    fo = str(tmp_path / "out.mtx")
    dt, semiring, bt = np.float64, "plus_times", form in ("bt", "plus_pair_bt")
    A = sr.csr(N, M, *m["A"][2])
    B, p, S = sr.csr(M, P, *m["B"][2]), P, m["S"]
    args = [f["A"], "0", "--B", f["Bt"] if bt else f["B"], "--sampled", f["S"], "--out", fo] + (["--sampled-bt"] if bt else [])
    if form == "max_plus":
        args += ["--semiring", "max_plus"]
        semiring = "max_plus"
    elif form == "plus_pair_bt":
        args += ["--semiring", "plus_pair"]
        semiring = "plus_pair"
    elif form == "fp32":
        args += ["--fp32"]
        dt = np.float32
    elif form == "AAt":
        args = [f["A"], "0", "1", "--sampled", f["SA"], "--out", fo]
        B, p, S = sr.transpose(N, M, A), N, m["SA"]
    out = _run(args, _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    assert out.stdout.count("sampled: R = pattern(S) o (A*B") == 1 and f"({semiring})" in out.stdout and "R written to" in out.stdout, out.stdout
    assert "SAMPLED AT" in out.stdout and "CLEANING UP RESOURCES" in out.stdout
    srp, sci, _ = sr.csr(S[0], S[1], S[2][0], S[2][1], S[2][2])
    I = sr.rows_of(srp)
    want = sr.sampled(I, sci, A, B, M, p, semiring, dt, oracle=oracle)
    gi, gj, gv = _read_coo(fo)
    # (a Matrix-Market reader may drop nothing: start values and zeros are entries of R)
    assert np.array_equal(gi, I) and np.array_equal(gj, sci), form
    assert _same(gv, want, dt), form


def test_triangles(standins, tmp_path):
    n, I, J = sr.triangle_graph(60, 400, 9)
    fa = str(tmp_path / "G.mtx")
    standins.write_mtx(fa, n, n, I, J, np.ones(len(I)))
    for extra in ([], ["--fp32"]):
        out = _run([fa, "0", "--triangles"] + extra, _env(tmp_path))
        assert out.returncode == 0, out.stderr + out.stdout
        assert f"triangles: {sr.triangles(n, I, J)} " in out.stdout, out.stdout


def test_shape_refusals(mats, tmp_path):
    m, f = mats
    env = _env(tmp_path)
    for args, word in (([f["A"], "0", "--B", f["B"], "--sampled", f["SA"]], f"is {N} x {N} but A*B is {N} x {P}"),
                       ([f["A"], "0", "--B", f["B"], "--sampled", f["S"], "--sampled-bt"], "inner dimensions differ"),
                       ([f["A"], "0", "--B", f["Bt"], "--sampled", f["SA"], "--sampled-bt"], f"but A*B^T is {N} x {P}"),
                       ([f["A"], "0", "--sampled", f["S"]], "rectangular"), ([f["A"], "0", "--triangles"], "rectangular"),
                       ([f["A"], "0", "--B", f["B"], "--sampled", str(tmp_path / "none.mtx")], "")):
        out = _run(args, env)
        assert out.returncode != 0 and word in out.stdout and "sampled:" not in out.stdout, (args, out.stdout, out.stderr)


def test_default_run_is_unchanged(pkg, ctx, mats, tmp_path):
    """no new flag: the plan product, its report lines and its --out as before"""
    m, f = mats
    fo = str(tmp_path / "c.mtx")
    out = _run([f["A"], "0", "--B", f["B"], "--out", fo], _env(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    assert "sampled" not in out.stdout.lower() and "triangles" not in out.stdout and "C written to" in out.stdout
    A = pkg.Tiled.from_coo(ctx, N, M, *m["A"][2])
    B = pkg.Tiled.from_coo(ctx, M, P, *m["B"][2])
    p = pkg.CPlan(ctx, A, B)
    p.spgemm()
    rp, ci, v = p.export_csr()
    gi, gj, gv = _read_coo(fo)
    assert np.array_equal(gi, sr.rows_of(rp)) and np.array_equal(gj, ci) and _same(gv, v, np.float64)
