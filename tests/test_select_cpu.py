"""CPU: tests/selectref.py against a per-entry brute force, over all 15 ops and both dtypes, with thunks that are negative, zero, beyond
the shape, +-0, +-inf and NaN, and values that are +-0, +-inf, NaN and subnormal; the package lists the ops and the built library
exports the select entry points."""
import math

import numpy as np
import pytest

import selectref as sel

SPECIAL = np.array([0.0, -0.0, 1.0, -1.0, 2.5, -2.5, np.inf, -np.inf, np.nan, 3.0e-310, -3.0e-310, 1.0e-40, 7.0])
POS_THUNKS = (0, 1, -1, 5, -7, 40, -40, 1000, -1000, 2 ** 31, -(2 ** 31), 0.0, -0.0)
VAL_THUNKS = (0.0, -0.0, 1.0, -1.0, 2.5, 0.1, np.inf, -np.inf, np.nan, 3.0e-310, 1.0e-40)


def _matrix(rng, rows, cols, n, dt):
    keys = np.sort(rng.choice(rows * cols, size=min(n, rows * cols), replace=False))
    V = np.where(rng.random(len(keys)) < 0.5, rng.choice(SPECIAL, len(keys)), rng.normal(size=len(keys)))
    return (keys // cols).astype(np.int32), (keys % cols).astype(np.int32), V.astype(dt)


def _brute_keep(op, i, j, x, thunk, dt):
    """one entry, plain Python: the header comment of pem_tiled_select"""
    i, j = int(i), int(j)
    if op in sel.POSITIONAL:
        k = int(thunk)
        return {"tril": j <= i + k, "triu": j >= i + k, "diag": j == i + k, "offdiag": j != i + k, "row_le": i <= k, "row_gt": i > k,
                "col_le": j <= k, "col_gt": j > k}[op]
    x = float(x)
    y = float(dt.type(thunk))   # (rounded once to the value type; exact as a Python float)
    if math.isnan(x) or math.isnan(y):
        return op == "value_ne"
    return {"value_eq": x == y, "value_ne": x != y, "value_lt": x < y, "value_le": x <= y, "value_gt": x > y, "value_ge": x >= y,
            "abs_gt": abs(x) > y}[op]


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
@pytest.mark.parametrize("op", sel.OPS)
def test_selectref_matches_brute_force(op, dtype):
    dt = np.dtype(dtype)
    rng = np.random.default_rng([sel.OPS.index(op), dt.itemsize])
    thunks = POS_THUNKS if op in sel.POSITIONAL else VAL_THUNKS
    for rows, cols, n in ((7, 9, 30), (40, 33, 500), (1, 50, 20), (50, 1, 20), (20, 20, 0)):
        I, J, V = _matrix(rng, rows, cols, n, dt)
        for thunk in thunks:
            kI, kJ, kV = sel.select(I, J, V, op, thunk, dt)
            assert kV.dtype == dt
            want = [e for e in range(len(I)) if _brute_keep(op, I[e], J[e], V[e], thunk, dt)]
            assert np.array_equal(kI, I[want]) and np.array_equal(kJ, J[want]), (op, thunk, rows, cols)
            assert np.array_equal(kV.view(np.uint8), V[want].view(np.uint8)), "values are not copied bit for bit"


def test_positional_thunk_rule():
    for k in (0, -3, 7, 2 ** 31, -(2 ** 31), 5.0, -0.0):
        assert sel.positional_thunk_ok(k)
    for k in (0.5, -1.25, 2.0 ** 31 + 1, -(2.0 ** 31) - 1, np.inf, -np.inf, np.nan, 1e300):
        assert not sel.positional_thunk_ok(k)
        with pytest.raises(ValueError):
            sel.select(np.zeros(1, np.int32), np.zeros(1, np.int32), np.ones(1), "tril", k)


def test_special_cases_spelled_out():
    I = np.zeros(8, np.int32)
    J = np.arange(8, dtype=np.int32)
    V = np.array([0.0, -0.0, np.nan, 1.0, -1.0, np.inf, -np.inf, 5e-324])
    assert list(sel.keep("value_ne", I, J, V, 0.0)) == [False, False, True, True, True, True, True, True]   # drop explicit zeros
    assert list(sel.keep("value_eq", I, J, V, -0.0)) == [True, True, False, False, False, False, False, False]
    assert list(sel.keep("abs_gt", I, J, V, 0.5)) == [False, False, False, True, True, True, True, False]   # NaN dropped
    assert sel.keep("value_ne", I, J, V, np.nan).all()
    for op in ("value_eq", "value_lt", "value_le", "value_gt", "value_ge", "abs_gt"):
        assert not sel.keep(op, I, J, V, np.nan).any()
    # fp32: the thunk is rounded once to float (0.1 -> 0.100000001490116...), the values compared as float
    x = np.array([np.float32(0.1)], np.float32)
    assert sel.keep("value_eq", [0], [0], x, 0.1, np.float32).all()
    assert not sel.keep("value_eq", [0], [0], x.astype(np.float64), 0.1, np.float64).any()
    # subnormal fp32 values are not flushed
    assert sel.keep("value_gt", [0], [0], np.array([1e-45], np.float32), 0.0, np.float32).all()


def test_package_lists_the_ops_and_library_exports_select(pkg):
    assert pkg.SELECT_OPS == sel.OPS
    assert len(pkg.SELECT_OPS) == 15
    for sym in ("pem_tiled_select", "pem_tiled_set_values_from_select"):
        assert sym in pkg.ABI_SYMBOLS
        assert hasattr(pkg.lib(), sym), f"the library does not export {sym}"
