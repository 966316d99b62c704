"""CPU: colourref, the host model of the graph colouring, proved on every graph the GPU tests use: the
golden values of the priority hash; the sequential greedy colouring in priority order equals the round-synchronous Jones-Plassmann
colouring, in colours, in every vertex's round and in the two counts; no stored off-diagonal entry joins two vertices of one colour;
equal priorities give tools/trsv_pass.py's natural-order greedy colouring; the figures the issue states for the graphs.  Also: the
header declares the two symbols, the library exports them, the binding refuses bad arguments before it touches a device, and the
CLI refuses what --colour does not combine with."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import colourref as cr
from matgen import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = cases()
NAMES = ("one_entry", "empty_matrix", "diag_100", "ragged_37", "dense_tile", "dense_48", "empty_rows", "rand_300", "powerlaw_600",
         "hub_row_4000", "band_1500")
GRAPHS = {name: (CASES[name][0], CASES[name][2], CASES[name][3]) for name in NAMES}
GRAPHS.update(cr.built_graphs())
SEEDS = (0, 12345)


def priorities(n, which):
    """the four priority settings of the GPU tests: the two seeds (None: hashed), all equal, random with many ties"""
    if which in SEEDS:
        return cr.hash_priority(n, which)
    if which == "equal":
        return np.zeros(n, np.uint32)
    return np.random.default_rng(n + 5).integers(0, 4, n).astype(np.uint32) * np.uint32(0x40000001)


def test_hash_golden_values():
    want = {0: (0x0, 0x514e28b7, 0x552553bc, 0x50a0dd96), 12345: (0xcf94c316, 0xcb6dd530, 0x0ffd6b2d, 0x853a7aed)}
    for seed, vals in want.items():
        got = tuple(cr.fmix32(v + seed * 0x9E3779B9) for v in (0, 1, 16, 1000004))
        assert got == vals, (seed, [hex(x) for x in got])
    p = cr.hash_priority(4096, 12345)
    assert len(np.unique(p)) == 4096 and p.dtype == np.uint32   # a bijection: no two vertices tie


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_greedy_is_jones_plassmann_and_valid(name):
    n, I, J = GRAPHS[name]
    Is, Js = cr.symmetrised(I, J) if len(I) else (I, J)
    for symmetric, (gi, gj) in ((False, (I, J)), (True, (Is, Js))):
        adj = cr.adjacency(n, gi, gj, symmetric)
        if symmetric:
            assert adj == cr.adjacency(n, I, J, False)   # the promise kept: the same graph
        for which in SEEDS + ("equal", "ties"):
            prio = priorities(n, which)
            colour, rnd, nc, rounds = cr.greedy(adj, prio)
            jc, jr, jnc, jrounds = cr.jones_plassmann(adj, prio)
            assert np.array_equal(colour, jc) and np.array_equal(rnd, jr) and (nc, rounds) == (jnc, jrounds), (name, which)
            assert cr.is_valid(n, I, J, colour) and nc == colour.max() + 1 and rounds == rnd.max() and rnd.min() >= 1
    if name == "path_203_one_way":   # the row orientation alone sees vertex i + 1 from i, never i from i + 1
        c1, nc1, r1 = cr.colouring(n, I, J, priority=np.zeros(n, np.uint32), symmetric=True)
        assert (nc1, r1) == (1, 1) and not cr.is_valid(n, I, J, c1)   # which is what a walk without the column direction would give


def test_the_figures_the_graphs_pin_down():
    def run(name, which):
        n, I, J = GRAPHS[name]
        return cr.colouring(n, I, J, priority=priorities(n, which))[1:]
    assert run("one_entry", 0) == (1, 1) and run("empty_matrix", 0) == (1, 1) and run("diag_100", 12345) == (1, 1)
    assert run("dense_tile", 0) == (16, 16) and run("dense_48", 12345) == (48, 48)
    assert run("hub_row_4000", 0) == (6, 14) and run("hub_row_4000", 12345) == (6, 16)
    assert run("band_1500", "equal")[1] == 270
    assert run("k70_in_75", 0) == (70, 70) and run("k131", "equal") == (131, 131)
    assert run("path_203_one_way", "equal") == (2, 203)
    assert run("path_203_one_way", 0) == (3, 5) and run("path_203_one_way", 12345) == (3, 6)
    n, I, J = GRAPHS["k70_in_75"]
    c, nc, rounds = cr.colouring(n, I, J, seed=0)
    assert np.all(c[70:] == 0) and sorted(c[:70]) == list(range(70))   # the isolated vertices take colour 0
    assert cr.colouring(0, np.zeros(0, np.int32), np.zeros(0, np.int32))[1:] == (0, 0)


@pytest.mark.parametrize("name", ("ragged_37", "rand_300", "powerlaw_600", "band_1500", "path_203_one_way"))
def test_equal_priorities_are_the_natural_greedy_colouring(name):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        trsv_pass = importlib.import_module("trsv_pass")
    finally:
        sys.path.pop(0)
    n, I, J = GRAPHS[name]
    Is, Js = cr.symmetrised(I, J)
    want = trsv_pass.greedy_colouring(n, Is.astype(np.int64), Js.astype(np.int64))
    got, nc, _ = cr.colouring(n, I, J, priority=np.full(n, 7, np.uint32))
    assert np.array_equal(got, want) and nc == want.max() + 1


def test_colour_order_model():
    rng = np.random.default_rng(4)
    c = rng.integers(0, 7, 1000).astype(np.int32)
    perm, off = cr.colour_order(c, 9)   # two colours nobody holds
    assert len(off) == 10 and off[0] == 0 and off[-1] == 1000 and off[7] == off[8] == 1000
    for k in range(9):
        seg = perm[off[k]:off[k + 1]]
        assert np.all(c[seg] == k) and np.all(np.diff(seg) > 0)


def test_header_library_and_binding(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pem_spgemm.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pem_[a-z0-9_]+)\s*\(", text))
    for sym in ("pem_tiled_colour", "pem_colour_order"):
        assert sym in declared and sym in pkg.ABI_SYMBOLS and hasattr(pkg.lib(), sym), sym
    for m in ("colour", "reorder_by_colour"):
        assert callable(getattr(pkg.Tiled, m))
    assert callable(pkg.colour_order)


def test_binding_refuses_before_the_device(pkg):
    """the host-side checks of Tiled.colour's seed and host priorities and of colour_order: ValueError, no device touched"""
    for seed in (-1, 2 ** 32, 1.5, "7", True, None):
        with pytest.raises(ValueError, match="seed"):
            pkg._colour_seed(seed)
    assert pkg._colour_seed(0) == 0 and pkg._colour_seed(np.int64(2 ** 32 - 1)) == 2 ** 32 - 1
    for bad, word in ((np.zeros(5), "integers"), (np.zeros(3, np.int64), "5 entries"), (np.zeros((5, 1), np.int32), "5 entries"),
                      (np.array([0, 1, 2, 3, -1]), "outside"), (np.array([0, 1, 2, 3, 2 ** 32]), "outside"),
                      (np.array([0.5] * 5), "integers")):
        with pytest.raises(ValueError, match=word):
            pkg._colour_priority(bad, 5)
    p = pkg._colour_priority([3, 2 ** 32 - 1, 0, 7, 7], 5)
    assert p.dtype == np.uint32 and p.tolist() == [3, 2 ** 32 - 1, 0, 7, 7]

    class NoCtx:
        device, _h = 0, None
    for colours, nc in ((np.zeros(4, np.int32), 1), ([0, 1], 2)):
        with pytest.raises(ValueError, match="int32 tensor"):
            pkg.colour_order(NoCtx(), colours, nc)
    import torch
    host = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="int32 tensor"):
        pkg.colour_order(NoCtx(), host, 1)             # not on the device
    for nc in (-1, 1.0, None, True, 2 ** 31):
        with pytest.raises(ValueError, match="ncolours"):
            pkg.colour_order(NoCtx(), host, nc)


def test_library_refuses_before_the_device(pkg):
    """PEM_E_INVALID for the arguments that need no context or tiling to be judged (the rest: tests/test_gpu_colour.py)"""
    import ctypes as C
    L = pkg.lib()
    nc, rounds = C.c_int32(5), C.c_int32(5)
    assert L.pem_tiled_colour(None, None, 0, C.c_uint32(0), None, C.c_void_p(256), C.byref(nc), C.byref(rounds)) == -1
    P = C.c_void_p
    order = lambda ctx=None, n=4, c=P(4096), k=2, p=P(8192), o=P(16384): L.pem_colour_order(ctx, C.c_int64(n), c, C.c_int32(k), p, o)
    assert order() == -1                                # a null context
    assert b"null" in L.pem_last_error()


def test_cli_refuses_before_it_opens_a_device(pkg, tmp_path):
    """--colour / --colour-natural: one line and exit code 1 for a bad seed and for what they do not combine with"""
    hostio = importlib.import_module("pem_spgemm_amd.hostio")
    fa = tmp_path / "A.mtx"
    fa.write_text("%%MatrixMarket matrix coordinate real general\n2 2 2\n1 1 1.0\n2 2 2.0\n")
    fx = tmp_path / "X.mtx"
    fx.write_text("%%MatrixMarket matrix array real general\n2 1\n1.0\n1.0\n")
    lines = [(["--colour", "x"], "--colour x: want a seed in 0 .. 4294967295. Exiting."),
             (["--colour", "-1"], "--colour -1: want a seed in 0 .. 4294967295. Exiting."),
             (["--colour", "4294967296"], "--colour 4294967296: want a seed in 0 .. 4294967295. Exiting."),
             (["--colour", "7", "--colour-natural"],
              "--colour does not combine with --colour-natural (a seed hashes the priorities, --colour-natural makes them equal). Exiting.")]
    for flag, spec in (("--colour", ["--colour", "7"]), ("--colour-natural", ["--colour-natural"])):
        for other, more in (("--gpus", ["2"]), ("--power", ["2"]), ("--reduce", ["rows"]), ("--bfs", ["1"]), ("--argreduce", ["rows:min"]),
                            ("--bfs-parents", ["1"]), ("--trsv", ["lower"]), ("--spmm", [str(fx)]), ("--sddmm", [str(fx)])):
            lines.append((spec + [other] + more, f"{flag} does not combine with {other}. Exiting."))
    for args, line in lines:
        out = subprocess.run([hostio.CLI_PATH, str(fa), "0", *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert out.returncode == 1 and out.stdout == line + "\n", (args, out.stdout, out.stderr)
