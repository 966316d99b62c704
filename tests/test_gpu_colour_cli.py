"""GPU: `pemspgemm A.mtx 0 --colour SEED [--out colours.mtx]` and `--colour-natural` (the greedy colouring of the final result's
pattern on the device) against colourref on the same pattern -- C = A*A of a small golden .mtx, and the
strict upper triangle of a golden product (every edge stored one way); and their refusals, each one line and exit code 1."""
import importlib
import os
import subprocess

import numpy as np
import pytest
import torch

import colourref as cr

pytestmark = pytest.mark.gpu

torch.cuda.is_available()

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CAGE4 = os.path.join(GOLDEN, "mm_cage4_standin.mtx")


def _run(args, env):
    hostio = importlib.import_module("pem_spgemm_amd.hostio")
    return subprocess.run([hostio.CLI_PATH, *args], env=env, capture_output=True, text=True, timeout=120)


def _env(tmp_path, name="r.csv"):
    return dict(os.environ, PEM_CSV=str(tmp_path / name), PEM_REPEAT="2")


def _read_ints(path):
    lines = open(path).read().splitlines()
    assert lines[0].split() == ["%%MatrixMarket", "matrix", "array", "integer", "general"]
    body = [ln for ln in lines if not ln.startswith("%")]
    assert body[0].split() == [str(len(body) - 1), "1"]
    return np.array([int(x) for x in body[1:]], np.int32)


def _cage4_square():
    """(n, I, J): the structural pattern of C = A*A of the golden 9 x 9 file"""
    body = [ln.split() for ln in open(CAGE4).read().splitlines() if not ln.startswith("%")]
    n = int(body[0][0])
    P = np.zeros((n, n), np.int64)
    for i, j, _ in body[1:]:
        P[int(i) - 1, int(j) - 1] = 1
    I, J = np.nonzero(P @ P)
    return n, I.astype(np.int32), J.astype(np.int32)


def _rand300_upper(standins, tmp_path):
    """(file, n, I, J): the golden rand_300 input written out, and the strict upper triangle of its golden product's pattern"""
    z = np.load(os.path.join(GOLDEN, "spgemm_rand_300.npz"))
    n = int(z["rows"])
    fa = str(tmp_path / "rand_300.mtx")
    standins.write_mtx(fa, n, n, z["I"], z["J"], z["V"])
    I = np.repeat(np.arange(n, dtype=np.int32), np.diff(z["c_rowptr"]))
    J = np.asarray(z["c_colidx"], np.int32)
    up = J > I
    return fa, n, I[up], J[up]


@pytest.mark.parametrize("fp32", (False, True), ids=("f64", "f32"))
def test_colour_matches_the_model(tmp_path, fp32):
    n, I, J = _cage4_square()
    for args, prio, label in ((["--colour", "12345"], cr.hash_priority(n, 12345), "seed 12345"), (["--colour", "0"], cr.hash_priority(n, 0), "seed 0"),
                              (["--colour-natural"], np.zeros(n, np.uint32), "natural order")):
        fc = str(tmp_path / "colours.mtx")
        out = _run([CAGE4, "0", *args, "--out", fc] + (["--fp32"] if fp32 else []), _env(tmp_path))
        assert out.returncode == 0, out.stderr + out.stdout
        c, nc, rounds = cr.colouring(n, I, J, priority=prio)
        assert out.stdout.count("colour: ") == 1 and f"colour: {label} of C: {nc} colours in {rounds} rounds, {n} vertices, colour " in out.stdout, out.stdout
        assert "colours written to" in out.stdout
        assert np.array_equal(_read_ints(fc), c + 1)
        row = (tmp_path / "r.csv").read_text().strip().splitlines()[-1].split(",")
        assert len(row) == 22   # (the CSV row keeps its width: it describes the product)


def test_after_select_and_without_out(standins, tmp_path):
    fa, n, I, J = _rand300_upper(standins, tmp_path)
    assert len(I) > 1000
    fc = str(tmp_path / "colours.mtx")
    for args, prio, label in ((["--colour", "12345"], cr.hash_priority(n, 12345), "seed 12345"), (["--colour-natural"], np.zeros(n, np.uint32), "natural order")):
        c, nc, rounds = cr.colouring(n, I, J, priority=prio)
        assert nc > 3 and cr.is_valid(n, I, J, c)
        out = _run([fa, "0", "--select", "triu:1", *args, "--out", fc], _env(tmp_path))
        assert out.returncode == 0, out.stderr + out.stdout
        assert f"colour: {label} of the selection: {nc} colours in {rounds} rounds, {n} vertices, colour " in out.stdout, out.stdout
        assert np.array_equal(_read_ints(fc), c + 1)
        out = _run([fa, "0", "--select", "triu:1", *args], _env(tmp_path))
        assert out.returncode == 0 and f"colour: {label} of the selection: {nc} colours in {rounds} rounds" in out.stdout and "written" not in out.stdout


def test_refusals(standins, tmp_path):
    env = _env(tmp_path)
    fx = str(tmp_path / "X.mtx")   # (a well-formed dense operand: the refusal is the combination's, not the file's)
    with open(fx, "w") as f:
        f.write("%%MatrixMarket matrix array real general\n9 1\n" + "1.0\n" * 9)
    frect = str(tmp_path / "R.mtx")
    standins.write_mtx(frect, 9, 4, np.array([0, 3, 8], np.int32), np.array([0, 1, 3], np.int32), np.ones(3))
    lines = [(["--colour", "x"], "--colour x: want a seed in 0 .. 4294967295. Exiting."),
             (["--colour", ""], "--colour : want a seed in 0 .. 4294967295. Exiting."),
             (["--colour", "-1"], "--colour -1: want a seed in 0 .. 4294967295. Exiting."),
             (["--colour", "1.5"], "--colour 1.5: want a seed in 0 .. 4294967295. Exiting."),
             (["--colour", "4294967296"], "--colour 4294967296: want a seed in 0 .. 4294967295. Exiting."),
             (["--colour", "7", "--colour-natural"],
              "--colour does not combine with --colour-natural (a seed hashes the priorities, --colour-natural makes them equal). Exiting.")]
    for flag, spec in (("--colour", ["--colour", "7"]), ("--colour-natural", ["--colour-natural"])):
        for other, more in (("--gpus", ["2"]), ("--power", ["3"]), ("--reduce", ["rows"]), ("--bfs", ["1"]), ("--argreduce", ["rows:min"]),
                            ("--bfs-parents", ["1"]), ("--trsv", ["lower"]), ("--spmm", [fx]), ("--sddmm", [fx])):
            lines.append((spec + [other] + more, f"{flag} does not combine with {other}. Exiting."))
    for args, line in lines:
        out = _run([CAGE4, "0"] + args, env)
        assert out.returncode == 1 and out.stdout == line + "\n", (args, out.stdout, out.stderr)
    assert not os.path.exists(tmp_path / "r.csv")
    for flag, spec in (("--colour", ["--colour", "7"]), ("--colour-natural", ["--colour-natural"])):
        out = _run([CAGE4, "0", "--B", frect] + spec, env)   # C = A * B is 9 x 4: known only once the result exists
        assert out.returncode == 1 and out.stdout.splitlines()[-1] == f"{flag}: C is 9 x 4; a colouring needs a square matrix. Exiting.", out.stdout
