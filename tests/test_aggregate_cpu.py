"""CPU: aggref, the host model of the independent sets and the aggregation, proved on every graph the GPU
tests use, under the two seeds, all-equal priorities and test_gpu_colour.py's "ties" array: the round-synchronous model equals the
sequential greedy set at both distances; the set is independent and maximal at its distance; the distance-1 set is colour 0 of
colourref's greedy colouring; every aggregate holds one root, every member lies within 2 of it inside the aggregate, nothing keeps
-1, the ids ascend by root; the figures the issue states for the graphs.  Also: the header declares the two symbols, the library
exports them, the binding carries their argtypes and refuses bad arguments before it touches a device, and the CLI refuses what
--aggregate does not combine with."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import aggref as ar
import colourref as cr
from matgen import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAPHS = ar.graphs(cases())
SEEDS = (0, 12345)
PRIORITIES = SEEDS + ("equal", "ties")


def test_beat_keys_order_the_vertices_as_beats_does():
    prio = np.array([0xFFFFFFFF, 5, 5, 0, 0xFFFFFFFF, 7], np.uint32)
    key = ar.beat_keys(prio)
    order, _ = cr._ranks(prio)
    assert np.argsort(-key.astype(object)).tolist() == order == [0, 4, 5, 1, 2, 3]
    assert key.min() >= 1 and key.max() < ar.IN_KEY and int(key[0]) == 2 ** 63   # the largest key there is stays below "in"


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_rounds_are_greedy_and_the_sets_are_maximal_independent(name):
    n, I, J = GRAPHS[name]
    Is, Js = cr.symmetrised(I, J) if len(I) else (I, J)
    adj = cr.adjacency(n, I, J)
    assert cr.adjacency(n, Is, Js, True) == adj                   # the promise kept: the same graph
    for which in PRIORITIES:
        prio = ar.priority_array(n, which)
        for distance in (1, 2):
            s, count, rounds = ar.mis(n, I, J, distance, priority=prio)
            assert np.array_equal(s, ar.greedy_mis(adj, prio, distance)), (name, which, distance)
            assert ar.is_mis(adj, s, distance) and count == s.sum() and 1 <= rounds <= n
            on_s = ar.mis(n, Is, Js, distance, priority=prio, symmetric=True)
            assert np.array_equal(on_s[0], s) and on_s[1:] == (count, rounds)
            if distance == 1:
                assert np.array_equal(s, (cr.greedy(adj, prio)[0] == 0).astype(np.uint8)), (name, which)
        isolated = np.array([len(a) == 0 for a in adj], bool)
        assert np.all(s[isolated] == 1)


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_aggregates(name):
    n, I, J = GRAPHS[name]
    adj = cr.adjacency(n, I, J)
    for which in PRIORITIES:
        prio = ar.priority_array(n, which)
        agg, roots, nc, rounds = ar.aggregate(n, I, J, priority=prio)
        s, count, r2 = ar.mis(n, I, J, 2, priority=prio)
        assert (nc, rounds) == (count, r2) and np.array_equal(roots, np.flatnonzero(s))
        ar.check_aggregation(adj, agg, roots, nc)
        for v in range(n):
            if not adj[v]:
                assert roots[agg[v]] == v and np.count_nonzero(agg == agg[v]) == 1


def test_hashed_seeds_are_what_a_priority_array_of_the_hash_gives():
    n, I, J = GRAPHS["rand_300"]
    for seed in SEEDS:
        a = ar.aggregate(n, I, J, seed=seed)
        b = ar.aggregate(n, I, J, priority=cr.hash_priority(n, seed))
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


FIGURES = [   # (graph, priorities, (distance-1 set, rounds), (aggregates, rounds), largest aggregate): the issue's table
    ("hub_row_4000", 0, (1842, 7), (1, 2), 4000), ("hub_row_4000", 12345, (1819, 8), (1, 2), 4000),
    ("band_1500", 0, (205, 11), (17, 6), 119), ("band_1500", "equal", (222, 58), (22, 42), 159),
    ("path_203_one_way", 12345, (87, 6), (59, 4), 5), ("path_203_one_way", "equal", (102, 203), (68, 136), 3),
    ("powerlaw_600", 0, (225, 8), (41, 12), 137), ("rand_300", 12345, (60, 7), (14, 10), 39), ("empty_rows", 0, (101, 4), (62, 6), 12),
    ("grid_40_one_way", 0, (594, 7), (233, 10), 11), ("grid_40_one_way", "equal", (800, 79), (280, 85), 7)]
for _name in ("empty_matrix", "one_entry", "diag_100"):
    FIGURES += [(_name, w, (GRAPHS[_name][0], 1), (GRAPHS[_name][0], 1), 1) for w in PRIORITIES]
for _name in ("dense_tile", "dense_48", "k131"):
    FIGURES += [(_name, w, (1, 2), (1, 2), GRAPHS[_name][0]) for w in PRIORITIES]
FIGURES += [("k70_in_75", w, (6, 2), (6, 2), 70) for w in PRIORITIES]


def test_the_figures_the_graphs_pin_down():
    for name, which, d1, aggs, largest in FIGURES:
        n, I, J = GRAPHS[name]
        prio = ar.priority_array(n, which)
        assert ar.mis(n, I, J, 1, priority=prio)[1:] == d1, (name, which)
        agg, _, nc, rounds = ar.aggregate(n, I, J, priority=prio)
        assert (nc, rounds) == aggs and np.bincount(agg).max() == largest, (name, which)
    z = np.zeros(0, np.int32)
    assert ar.mis(0, z, z, 1)[1:] == (0, 0) and ar.mis(0, z, z, 2)[1:] == (0, 0) and ar.aggregate(0, z, z)[2:] == (0, 0)


def test_a_false_promise_in_the_model_stays_in_bounds():
    n, I, J = GRAPHS["path_203_one_way"]
    for which in PRIORITIES:
        prio = ar.priority_array(n, which)
        s, count, rounds = ar.mis(n, I, J, 2, priority=prio, symmetric=True)
        agg, roots, nc, _ = ar.aggregate(n, I, J, priority=prio, symmetric=True)
        assert set(np.unique(s)) <= {0, 1} and rounds <= n and agg.min() >= -1 and agg.max() < nc == count


def test_header_library_and_binding(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pem_spgemm.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pem_[a-z0-9_]+)\s*\(", text))
    L = pkg.lib()
    for sym in ("pem_tiled_mis", "pem_tiled_aggregate"):
        assert sym in declared and sym in pkg.ABI_SYMBOLS and hasattr(L, sym), sym
    assert L.pem_tiled_mis.argtypes == [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p,
                                        C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    assert L.pem_tiled_aggregate.argtypes == [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    for m in ("mis", "aggregate"):
        assert callable(getattr(pkg.Tiled, m))
    assert callable(pkg.prolongator)


def test_library_and_binding_refuse_before_the_device(pkg):
    L = pkg.lib()
    count, rounds = C.c_int64(5), C.c_int32(5)
    assert L.pem_tiled_mis(None, None, 2, 0, 0, None, C.c_void_p(256), C.byref(count), C.byref(rounds)) == -1
    assert b"null" in L.pem_last_error()
    assert L.pem_tiled_aggregate(None, None, 0, 0, None, C.c_void_p(256), None, C.byref(count), C.byref(rounds)) == -1
    assert (count.value, rounds.value) == (5, 5)
    for seed in (-1, 2 ** 32, 1.5, True):
        with pytest.raises(ValueError, match="mis: seed"):
            pkg._colour_seed(seed, "mis")
    with pytest.raises(ValueError, match="aggregate: priority must hold 5 entries"):
        pkg._colour_priority(np.zeros(3, np.int64), 5, "aggregate")

    class NoCtx:
        device, _h = 0, None
    import torch
    with pytest.raises(ValueError, match="int32 tensor"):
        pkg.prolongator(NoCtx(), torch.zeros(4, dtype=torch.int32), 2)      # not on the device
    with pytest.raises(ValueError, match="int32 tensor"):
        pkg.prolongator(NoCtx(), np.zeros(4, np.int32), 2)
    for nc in (-1, 1.0, None, True, 2 ** 31):
        with pytest.raises(ValueError, match="naggregates"):
            pkg.prolongator(NoCtx(), torch.zeros(4, dtype=torch.int32), nc)


def test_cli_refuses_before_it_opens_a_device(pkg, tmp_path):
    """--aggregate: one line and exit code 1 for a bad seed and for what it does not combine with"""
    hostio = importlib.import_module("pem_spgemm_amd.hostio")
    fa = tmp_path / "A.mtx"
    fa.write_text("%%MatrixMarket matrix coordinate real general\n2 2 2\n1 1 1.0\n2 2 2.0\n")
    fx = tmp_path / "X.mtx"
    fx.write_text("%%MatrixMarket matrix array real general\n2 1\n1.0\n1.0\n")
    lines = [(["--aggregate", bad], f"--aggregate {bad}: want a seed in 0 .. 4294967295. Exiting.") for bad in ("x", "-1", "1.5", "4294967296")]
    for other, more in (("--gpus", ["2"]), ("--power", ["2"]), ("--reduce", ["rows"]), ("--bfs", ["1"]), ("--argreduce", ["rows:min"]),
                        ("--bfs-parents", ["1"]), ("--trsv", ["lower"]), ("--spmm", [str(fx)]), ("--sddmm", [str(fx)]), ("--colour", ["3"]),
                        ("--colour-natural", []), ("--components", [])):
        lines.append((["--aggregate", "7", other] + more, f"--aggregate does not combine with {other}. Exiting."))
    for args, line in lines:
        out = subprocess.run([hostio.CLI_PATH, str(fa), "0", *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert out.returncode == 1 and out.stdout == line + "\n", (args, out.stdout, out.stderr)
