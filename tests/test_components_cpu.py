"""CPU: the host model of the connected components (tests/ccref.py: the rounds of pem_tiled_components in numpy) against scipy, the
figures the contract pins down for the fixed graphs, the dense ids, and what is checkable without a device: the header, the binding
and the CLI's refusals of --components next to what it does not combine with."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import ccref as cc
from matgen import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = cases()
NAMES = ("one_entry", "empty_matrix", "diag_100", "tiny_9x9", "rand_50", "ragged_37", "dense_tile", "dense_48", "empty_rows", "rand_300",
         "powerlaw_600", "hub_row_4000", "band_1500")
GRAPHS = {name: (CASES[name][0], CASES[name][2], CASES[name][3]) for name in NAMES}
GRAPHS.update(cc.built_graphs())

# (components, rounds) of the fixed graphs: matgen's, colourref's and the deterministic ones
FIGURES = {"one_entry": (5, 1), "empty_matrix": (40, 1), "diag_100": (100, 1), "tiny_9x9": (1, 3), "rand_50": (1, 4), "ragged_37": (1, 3),
           "dense_tile": (1, 2), "dense_48": (1, 2), "empty_rows": (25, 5), "rand_300": (1, 4), "powerlaw_600": (1, 4), "hub_row_4000": (1, 3),
           "band_1500": (1, 6), "k70_in_75": (6, 2), "k131": (1, 2), "path_203_one_way": (1, 9), "path_4097_down": (1, 14),
           "star_in_2000": (2, 3)}


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_model_equals_scipy(name):
    n, I, J = GRAPHS[name]
    labels, rounds = cc.components_model(n, I, J)
    assert labels.dtype == np.int32 and np.array_equal(labels, cc.components_scipy(n, I, J))
    assert 1 <= rounds <= n and np.all(labels <= np.arange(n)) and np.all(labels[labels] == labels)
    # the row orientation alone sees the same graph once the pattern is united with its transpose
    Is, Js = cc.symmetrised(I, J) if len(I) else (I, J)
    l1, r1 = cc.components_model(n, Is, Js, symmetric_walk=True)
    l0, r0 = cc.components_model(n, Is, Js, symmetric_walk=False)
    assert np.array_equal(l1, labels) and r1 == rounds and np.array_equal(l0, labels) and r0 == rounds
    ids, nc = cc.ids_of(labels)
    roots = np.flatnonzero(labels == np.arange(n))
    assert nc == len(roots) and np.array_equal(ids, np.searchsorted(roots, labels).astype(np.int32))
    assert ids.dtype == np.int32 and (n == 0 or (ids.min() == 0 and ids.max() == nc - 1))
    if name in FIGURES:
        assert (nc, rounds) == FIGURES[name]


def test_the_figures_cover_the_fixed_graphs():
    assert set(FIGURES) <= set(GRAPHS) and len(FIGURES) == 18
    assert set(GRAPHS) - set(FIGURES) == {"path_5000_shuffled", "grid_64_shuffled", "sparse_forest_3000", "two_cycles_1025", "hyper_4194321"}


def test_the_built_graphs_are_what_they_say():
    G = cc.built_graphs()
    n, I, J = G["path_4097_down"]
    assert n == 4097 and np.array_equal(I, J + 1) and len(I) == 4096
    n, I, J = G["star_in_2000"]
    assert n == 2000 and np.all(J == 1999) and np.array_equal(I, np.arange(1, 2000))
    assert cc.ids_of(cc.components_scipy(n, I, J))[1] == 2 and cc.components_scipy(n, I, J)[0] == 0
    n, I, J = G["two_cycles_1025"]
    assert cc.ids_of(cc.components_scipy(n, I, J))[1] == 2 and sorted(np.bincount(cc.components_scipy(n, I, J), minlength=n)[:n].tolist())[-2:] == [500, 525]
    n, I, J = G["grid_64_shuffled"]
    assert n == 4096 and len(I) == 2 * 64 * 63 and cc.ids_of(cc.components_scipy(n, I, J))[1] == 1
    n, I, J = G["hyper_4194321"]
    assert n == 2 ** 22 + 17 and n // 16 > 262144 and 2900 < len(I) <= 3000
    n, I, J = G["sparse_forest_3000"]
    assert n == 3000 and 1190 < len(I) <= 1200
    again = cc.built_graphs()
    for name in G:
        assert G[name][0] == again[name][0] and np.array_equal(G[name][1], again[name][1]) and np.array_equal(G[name][2], again[name][2])


def test_a_false_promise_in_the_model_stays_in_bounds():
    n, I, J = GRAPHS["path_203_one_way"]
    labels, rounds = cc.components_model(n, I, J, symmetric_walk=True)
    assert np.all(labels >= 0) and np.all(labels <= np.arange(n)) and 1 <= rounds <= n


def test_header_declares_the_call():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pem_spgemm.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pem_[a-z0-9_]+)\s*\(", text))
    assert "pem_tiled_components" in declared and "pem_component_order" not in declared


def test_library_and_binding(pkg):
    assert "pem_tiled_components" in pkg.ABI_SYMBOLS and hasattr(pkg.lib(), "pem_tiled_components")
    for m in ("components", "reorder_by_component"):
        assert callable(getattr(pkg.Tiled, m))
    # PEM_E_INVALID for what needs no context or tiling to be judged (the rest: tests/test_gpu_components.py)
    import ctypes as C
    nc, rounds = C.c_int64(5), C.c_int32(5)
    assert pkg.lib().pem_tiled_components(None, None, 0, C.c_void_p(256), None, C.byref(nc), C.byref(rounds)) == -1
    assert b"null" in pkg.lib().pem_last_error() and (nc.value, rounds.value) == (5, 5)


def test_cli_refuses_before_it_opens_a_device(pkg, tmp_path):
    """--components: one line and exit code 1 for what it does not combine with (a result that is not square is known only once it
    exists: tests/test_gpu_components_cli.py)"""
    hostio = importlib.import_module("pem_spgemm_amd.hostio")
    fa = tmp_path / "A.mtx"
    fa.write_text("%%MatrixMarket matrix coordinate real general\n2 2 2\n1 1 1.0\n2 2 2.0\n")
    fx = tmp_path / "X.mtx"
    fx.write_text("%%MatrixMarket matrix array real general\n2 1\n1.0\n1.0\n")
    lines = []
    for other, more in (("--colour", ["7"]), ("--colour-natural", []), ("--trsv", ["lower"]), ("--gpus", ["2"]), ("--power", ["2"]),
                        ("--reduce", ["rows"]), ("--bfs", ["1"]), ("--argreduce", ["rows:min"]), ("--bfs-parents", ["1"]), ("--spmm", [str(fx)]),
                        ("--sddmm", [str(fx)])):
        lines.append((["--components", other] + more, f"--components does not combine with {other}. Exiting."))
        lines.append(([other] + more + ["--components"], f"--components does not combine with {other}. Exiting."))
    for args, line in lines:
        out = subprocess.run([hostio.CLI_PATH, str(fa), "0", *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert out.returncode == 1 and out.stdout == line + "\n", (args, out.stdout, out.stderr)
