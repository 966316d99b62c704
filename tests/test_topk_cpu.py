"""CPU: the yardstick of select top-k (tests/topkref.py) against a brute force written from the three rules of the rank order
(include/pem_spgemm.h, pem_tiled_select_topk), its invariants, and what the binding and the CLI refuse without a device."""
import functools
import importlib
import math
import subprocess

import numpy as np
import pytest

import topkref as tk
from matgen import cases

CASES = cases()
DTYPES = (np.float64, np.float32)
KS = (0, 1, 2, 15, 16, 17, 64, 10 ** 6)
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3.0e-310, 1.0e-40, 0.5, -0.5])


def _with_specials(case, seed=3):
    """the case's values with about a fifth replaced by +-0, +-inf, NaN and subnormals (as tests/test_gpu_select.py does)"""
    rows, cols, I, J, V, _ = case
    rng = np.random.default_rng(seed + rows * 7 + cols)
    W = np.array(V, np.float64)
    sp = rng.random(len(W)) < 0.2
    W[sp] = rng.choice(SPECIAL, int(sp.sum()))
    return W


def _cmp(order):
    """a before b (< 0) in the rank order of a line; a, b = (value is a NaN, value as a Python float (0.0 for a NaN), index inside
    the line, ...).  IEEE comparisons: -0.0 == 0.0, and a float32 compares as the double it converts to exactly."""
    def rule3(a, b):                       # equal entries, and NaNs among themselves: the lower index first
        return a[2] - b[2]

    def largest(a, b):
        if a[0] != b[0]:                   # rule 1: numbers before NaNs
            return 1 if a[0] else -1
        if a[1] != b[1]:                   # rule 2
            return -1 if a[1] > b[1] else 1
        return rule3(a, b)

    def smallest(a, b):
        if a[0] != b[0]:
            return 1 if a[0] else -1
        if a[1] != b[1]:
            return -1 if a[1] < b[1] else 1
        return rule3(a, b)

    def abs_largest(a, b):
        if a[0] != b[0]:
            return 1 if a[0] else -1
        if abs(a[1]) != abs(b[1]):
            return -1 if abs(a[1]) > abs(b[1]) else 1
        return rule3(a, b)

    return dict(largest=largest, smallest=smallest, abs_largest=abs_largest)[order]


def _lines(I, J, V, dim):
    """line -> [(is a NaN, value (0.0 for a NaN), index inside the line, position in the triple)]"""
    line, idx = (I, J) if dim == "rows" else (J, I)
    nan = np.isnan(V)
    out = {}
    for p, (l, x, n, v) in enumerate(zip(line.tolist(), idx.tolist(), nan.tolist(), np.where(nan, 0, V).tolist())):
        out.setdefault(l, []).append((n, v, x, p))
    return out


def _brute_ranks(I, J, V, order, dim):
    """rank of every entry inside its line (0 = first), by sorting every line with the comparison"""
    key = functools.cmp_to_key(_cmp(order))
    rank = np.zeros(len(V), np.int64)
    for ents in _lines(I, J, V, dim).values():
        for r, e in enumerate(sorted(ents, key=key)):
            rank[e[3]] = r
    return rank


@pytest.mark.parametrize("order", tk.ORDERS)
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", sorted(CASES))
def test_topkref_equals_brute_force(name, dtype, order):
    rows, cols, I, J, V, _ = CASES[name]
    Vd = _with_specials(CASES[name]).astype(dtype)
    for dim in tk.DIMS:
        rank = _brute_ranks(I, J, Vd, order, dim)
        for k in KS:
            got = tk.keep(I, J, Vd, order, dim, k, dtype)
            assert np.array_equal(got, rank < k), f"{name} {order} {dim} k={k}: {int((got != (rank < k)).sum())} entries differ"
        kI, kJ, kV = tk.select_topk(I, J, Vd, order, dim, 2, dtype)   # the triple: the kept entries in input order, bit for bit
        got = rank < 2
        assert np.array_equal(kI, I[got]) and np.array_equal(kJ, J[got]) and kV.dtype == np.dtype(dtype)
        assert np.array_equal(kV.view(np.uint8), Vd[got].view(np.uint8)), f"{name} {order} {dim}: values not copied bit for bit"


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", ("tiny_9x9", "rand_300", "rect_33x65_AAt", "ragged_37", "dense_48", "empty_rows", "empty_matrix",
                                  "row_vector_AAt", "col_vector_AAt", "cancel_and_zero", "powerlaw_600", "hub_row_4000"))
def test_invariants(name, dtype):
    rows, cols, I, J, V, _ = CASES[name]
    Vd = _with_specials(CASES[name]).astype(dtype)
    nan = np.isnan(Vd)
    for order in tk.ORDERS:
        cmp = functools.cmp_to_key(_cmp(order))
        for dim in tk.DIMS:
            line = (I if dim == "rows" else J).astype(np.int64)
            nl = rows if dim == "rows" else cols
            n_line = np.bincount(line, minlength=nl)
            lines = _lines(I, J, Vd, dim)
            for k in KS:
                m = tk.keep(I, J, Vd, order, dim, k, dtype)
                label = f"{name} {order} {dim} k={k}"
                assert np.array_equal(np.bincount(line[m], minlength=nl), np.minimum(n_line, k)), f"{label}: not min(k, n_line) per line"
                nan_kept = np.bincount(line[m & nan], minlength=nl) > 0
                num_dropped = np.bincount(line[~m & ~nan], minlength=nl) > 0
                assert not np.any(nan_kept & num_dropped), f"{label}: a NaN kept while a number of its line is dropped"
                for ents in lines.values():
                    kept = [e for e in ents if m[e[3]]]
                    dropped = [e for e in ents if not m[e[3]]]
                    if kept and dropped:
                        assert cmp(max(kept, key=cmp)) < cmp(min(dropped, key=cmp)), f"{label}: a dropped entry ranks before a kept one"
                if k == 0:
                    assert not m.any(), label
                if k == 10 ** 6:
                    assert m.all(), label


def test_key_rules_by_hand():
    one = np.zeros(3, np.int32)
    j = np.arange(3, dtype=np.int32)
    for order in tk.ORDERS:   # both zeros before the NaN, in index order
        assert tk.keep(one, j, [0.0, np.nan, -0.0], order, "rows", 2).tolist() == [True, False, True]
        assert tk.keep(one, j, [0.0, -0.0, 0.0], order, "rows", 1).tolist() == [True, False, False]
        assert tk.keep(one, j, [np.nan, np.nan, 1.0], order, "rows", 2).tolist() == [True, False, True]
        assert tk.keep(j, one, [np.nan, -np.nan, np.nan], order, "cols", 2).tolist() == [True, True, False]
    v = [-np.inf, np.inf, 5e-324, -5e-324, 0.0]
    z = np.zeros(5, np.int32)
    i5 = np.arange(5, dtype=np.int32)
    assert [int(np.flatnonzero(tk.keep(z, i5, v, "largest", "rows", k) & ~tk.keep(z, i5, v, "largest", "rows", k - 1))[0])
            for k in range(1, 6)] == [1, 2, 4, 3, 0]
    assert [int(np.flatnonzero(tk.keep(z, i5, v, "smallest", "rows", k) & ~tk.keep(z, i5, v, "smallest", "rows", k - 1))[0])
            for k in range(1, 6)] == [0, 3, 4, 2, 1]
    assert [int(np.flatnonzero(tk.keep(z, i5, v, "abs_largest", "rows", k) & ~tk.keep(z, i5, v, "abs_largest", "rows", k - 1))[0])
            for k in range(1, 6)] == [0, 1, 2, 3, 4]
    # in float32 the fp64 subnormals are zeros: ties by index
    assert tk.keep(z, i5, v, "largest", "rows", 3, np.float32).tolist() == [False, True, True, True, False]
    with pytest.raises(ValueError):
        tk.keep(z, i5, v, "biggest", "rows", 1)
    with pytest.raises(ValueError):
        tk.keep(z, i5, v, "largest", "diag", 1)
    with pytest.raises(ValueError):
        tk.keep(z, i5, v, "largest", "rows", -1)


# ---- the binding's refusals that need no device ------------------------------------------------------------------------------
def test_binding_value_errors(pkg):
    assert pkg.TOPK_ORDERS == tk.ORDERS
    assert "pem_tiled_select_topk" in pkg.ABI_SYMBOLS
    none = object.__new__(pkg.Tiled)   # (no handle: every refusal below comes before the library is touched)
    for kwargs in (dict(k=1, order="biggest"), dict(k=1, order="largest", dim="diag"), dict(k=1, dim=0), dict(k=-1), dict(k=1.5),
                   dict(k=float("nan")), dict(k=float("inf")), dict(k="3"), dict(k=None), dict(k=True), dict(k=2 ** 63),
                   dict(k=np.float64(0.5)), dict(k=np.int64(-2))):
        with pytest.raises(ValueError):
            pkg.Tiled.select_topk(none, **kwargs)


# ---- the CLI's refusals, before a device is opened ---------------------------------------------------------------------------
FORM = "; the form is DIM:ORDER:K. Exiting.\n"
REFUSALS = (
    (["--topk", "cols:largest:3", "--gpus", "2"], "--topk does not combine with --gpus. Exiting.\n"),
    (["--topk", "cols:largest:3", "--power", "2"], "--topk does not combine with --power. Exiting.\n"),
    (["--topk", "diag:largest:3"], "--topk diag:largest:3: unknown dimension diag (rows, cols)" + FORM),
    (["--topk", "rows:biggest:3"], "--topk rows:biggest:3: unknown order biggest (largest, smallest, abs_largest)" + FORM),
    (["--topk", "rows"], "--topk rows: unknown order  (largest, smallest, abs_largest)" + FORM),
    (["--topk", "rows:largest:-1"], "--topk rows:largest:-1: K must be an integer >= 0, not -1. Exiting.\n"),
    (["--topk", "rows:largest:1.5"], "--topk rows:largest:1.5: K must be an integer >= 0, not 1.5. Exiting.\n"),
    (["--topk", "rows:largest:x"], "--topk rows:largest:x: K must be an integer >= 0, not x. Exiting.\n"),
    (["--topk", "rows:largest"], "--topk rows:largest: K must be an integer >= 0, not . Exiting.\n"),
    # an earlier step of the validation chain speaks first
    (["--select", "lower:0", "--topk", "rows:largest:x"],
     "--select lower:0: unknown op lower (tril, triu, diag, offdiag, row_le, row_gt, col_le, col_gt, value_eq, value_ne, value_lt, "
     "value_le, value_gt, value_ge, abs_gt). Exiting.\n"),
)


@pytest.mark.parametrize("k", range(len(REFUSALS)), ids=["_".join(a[0]).replace("--", "") for a in REFUSALS])
def test_cli_refusal(k, pkg, tmp_path):
    args, message = REFUSALS[k]
    hostio = importlib.import_module("pem_spgemm_amd.hostio")
    out = subprocess.run([hostio.CLI_PATH, "A.mtx", "0", *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert out.stdout == message
    assert out.returncode == 1, out.stderr
