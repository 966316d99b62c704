"""CPU: tests/buildref.py against independent statements -- a Python dict loop for every op and dtype, scipy's duplicate summation
for plus, a hand-written list for first and second -- plus the library's exports, the header's constants mirrored in the package, and
the command lines `pemspgemm --dup` refuses before it opens a device."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import buildref

DTYPES = (np.float64, np.float32)
IDS = ("f64", "f32")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pem_spgemm.h")
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 0.5, -2.0, 3.0])


def _scalar_ops(dt):
    return dict(plus=lambda a, b: a + b, times=lambda a, b: a * b, min=np.fmin, max=np.fmax,
                lor=lambda a, b: dt.type((a != 0) or (b != 0)), land=lambda a, b: dt.type((a != 0) and (b != 0)),
                first=lambda a, b: a, second=lambda a, b: b)


def _triplets(rng, rows, cols, n, dt, special):
    I = rng.integers(0, rows, n).astype(np.int32)
    J = rng.integers(0, cols, n).astype(np.int32)
    V = rng.normal(size=n).astype(dt)
    if special:
        pick = rng.random(n) < 0.3
        V[pick] = rng.choice(SPECIAL, int(pick.sum())).astype(dt)
    return I, J, V


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("transpose", (False, True), ids=("plain", "transposed"))
def test_fold_equals_a_dict_loop_for_every_op(dtype, transpose):
    dt = np.dtype(dtype)
    rng = np.random.default_rng(11)
    for rows, cols, n in ((4, 5, 60), (1, 1, 9), (7, 3, 0), (40, 40, 300)):
        I, J, V = _triplets(rng, rows, cols, n, dt, special=True)
        for op, f in _scalar_ops(dt).items():
            want = {}
            with np.errstate(all="ignore"):
                for i, j, v in zip(I, J, V):
                    pos = (int(j), int(i)) if transpose else (int(i), int(j))
                    want[pos] = dt.type(f(want[pos], v)) if pos in want else v
            oI, oJ, oV = buildref.fold(rows, cols, I, J, V, op, transpose)
            assert oV.dtype == dt and oI.dtype == oJ.dtype == np.int32
            assert [(int(i), int(j)) for i, j in zip(oI, oJ)] == sorted(want), (op, rows, cols)
            for i, j, v in zip(oI, oJ, oV):
                w = want[(int(i), int(j))]
                assert (np.isnan(v) and np.isnan(w)) or v.tobytes() == w.tobytes(), (op, i, j, v, w)
    with pytest.raises(ValueError):
        buildref.fold(4, 4, [0], [0], np.ones(1, dt), "avg")
    with pytest.raises(ValueError):
        buildref.fold(4, 4, [4], [0], np.ones(1, dt))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_plus_equals_scipys_duplicate_sum_on_small_integers(dtype):
    rng = np.random.default_rng(12)
    rows, cols, n = 50, 70, 4000
    I, J = rng.integers(0, rows, n), rng.integers(0, cols, n)
    V = rng.integers(-4, 5, n).astype(dtype)                      # every partial sum is exact: the order does not matter
    oI, oJ, oV = buildref.fold(rows, cols, I, J, V, "plus")
    M = sp.coo_matrix((V, (I, J)), shape=(rows, cols)).tocsr()    # (sums duplicates; keeps the zeros they cancel to)
    M.sort_indices()
    assert np.array_equal(np.repeat(np.arange(rows), np.diff(M.indptr)), oI) and np.array_equal(M.indices, oJ)
    assert np.array_equal(M.data, oV) and oV.dtype == np.dtype(dtype)


def test_first_and_second_on_a_hand_written_list():
    I = [2, 0, 2, 1, 0, 2, 1]
    J = [1, 0, 1, 3, 0, 1, 0]
    V = np.array([10.0, 20.0, 30.0, 40.0, 50.0, 60.0, 70.0])
    # positions in order: (0,0) <- 20, 50; (1,0) <- 70; (1,3) <- 40; (2,1) <- 10, 30, 60
    for op, want in (("first", [20.0, 70.0, 40.0, 10.0]), ("second", [50.0, 70.0, 40.0, 60.0]), ("plus", [70.0, 70.0, 40.0, 100.0]),
                     ("max", [50.0, 70.0, 40.0, 60.0])):
        oI, oJ, oV = buildref.fold(3, 4, I, J, V, op)
        assert oI.tolist() == [0, 1, 1, 2] and oJ.tolist() == [0, 0, 3, 1] and oV.tolist() == want, op
    tI, tJ, tV = buildref.fold(3, 4, I, J, V, "first", transpose=True)          # the 4 x 3 transpose, canonical
    assert tI.tolist() == [0, 0, 1, 3] and tJ.tolist() == [0, 1, 2, 1] and tV.tolist() == [20.0, 70.0, 10.0, 40.0]


def test_with_duplicates_keeps_the_positions_and_the_run_lengths():
    rng = np.random.default_rng(13)
    I, J = np.array([0, 0, 3, 5], np.int32), np.array([1, 2, 3, 0], np.int32)
    V = np.array([1.0, np.nan, -0.0, 4.0])
    lengths = [1, 4, 2, 3]
    tI, tJ, tV = buildref.with_duplicates(I, J, V, rng, lengths)
    assert len(tI) == 10
    order, start, key = buildref.runs(6, 4, tI, tJ)
    assert np.array_equal(key, I.astype(np.int64) * 4 + J) and np.diff(start).tolist() == lengths
    assert set(tV.view(np.uint64).tolist()) <= set(V.view(np.uint64).tolist())
    oI, oJ, oV = buildref.fold(6, 4, tI, tJ, tV, "first")
    assert np.array_equal(oI, I) and np.array_equal(oJ, J)


def test_library_exports_header_declares_and_package_mirrors_the_constants(pkg):
    syms = ("pem_tiled_build", "pem_tiled_build_f32", "pem_tiled_build_device", "pem_tiled_build_device_f32", "pem_tiled_set_values_from_build",
            "pem_tiled_set_values_from_build_f32")
    for sym in syms:
        assert sym in pkg.ABI_SYMBOLS
        assert hasattr(pkg.lib(), sym), f"the library does not export {sym}"
    text = open(HEADER).read()
    assert int(re.search(r"#define PEM_BUILD_INORDER_MAX (\d+)", text).group(1)) == pkg.BUILD_INORDER_MAX >= 32
    assert int(re.search(r"#define PEM_BUILD_KEEP_MAP (\d+)", text).group(1)) == pkg.BUILD_KEEP_MAP
    first, second = re.search(r"PEM_DUP_FIRST = (\d+), PEM_DUP_SECOND = (\d+)", text).groups()
    assert pkg.DUP_OPS == buildref.DUP_OPS == ("plus", "times", "min", "max", "lor", "land", "first", "second")
    assert pkg.DUP_OPS.index("first") == int(first) and pkg.DUP_OPS.index("second") == int(second)
    assert pkg.DUP_OPS[:6] == tuple(sorted(pkg.BINOPS, key=pkg.BINOPS.get))
    assert callable(pkg.Tiled.build) and callable(pkg.Tiled.build_device) and callable(pkg.Tiled.set_values_from_build)
    with pytest.raises(ValueError):
        pkg.Tiled.build(None, 1, 1, [0], [0], [1.0], dup="avg")


MTX = "%%MatrixMarket matrix coordinate real general\n2 2 3\n1 1 1.0\n1 1 2.0\n2 2 3.0\n"
REFUSALS = (
    (["a.mtx", "--dup", "avg"], "--dup avg: unknown op (plus, times, min, max, lor, land, first, second). Exiting.\n"),
    (["a.mtx", "--dup", "plus", "--gpus", "2"], "--dup does not combine with --gpus. Exiting.\n"),
    (["a.mtx", "--dup", "first", "--cache", "{tmp}"], "--dup does not combine with --cache. Exiting.\n"),
    (["a.mtx", "--cache", "{tmp}", "--dup", "avg"], "--dup avg: unknown op (plus, times, min, max, lor, land, first, second). Exiting.\n"),
    # an earlier check's refusal wins over --dup's: the order of the recorded refusals is unchanged
    (["a.mtx", "--dup", "avg", "--semiring", "upper"],
     "--semiring upper: unknown semiring (plus_times, min_plus, max_plus, max_times, plus_pair, lor_land). Exiting.\n"),
    (["a.mtx", "--dup", "plus", "--gpus", "2", "--power", "2"], "--power does not combine with --gpus (A^K multiplies A by itself on one device). Exiting.\n"),
)


@pytest.mark.parametrize("k", range(len(REFUSALS)), ids=[f"{k}" + "".join(a for a in r[0] if a.startswith("--")) for k, r in enumerate(REFUSALS)])
def test_cli_refusal(k, pkg, tmp_path):
    args, want = REFUSALS[k]
    hostio = importlib.import_module("pem_spgemm_amd.hostio")
    (tmp_path / "a.mtx").write_text(MTX)
    args = [a.replace("{tmp}", str(tmp_path)) for a in args]
    out = subprocess.run([hostio.CLI_PATH, *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert out.stdout == want
    assert out.returncode == 1, out.stderr
