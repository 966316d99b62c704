"""CPU: tests/ewiseref.py against a per-entry dict brute force, over every op, both patterns, both dtypes and (alpha, beta),
with explicit zeros, +-0, +-inf and NaN operands."""
import math

import numpy as np
import pytest

import ewiseref as er

SPECIAL = np.array([0.0, -0.0, 1.0, -2.5, np.inf, -np.inf, np.nan, 3.0e-310, 7.0])
SCALES = ((1.0, 1.0), (2.0, -0.5), (0.1, 3.0), (1.0, 0.0))


def _operand(rng, rows, cols, n, dt):
    keys = rng.choice(rows * cols, size=min(n, rows * cols), replace=False)
    keys.sort()
    V = np.where(rng.random(len(keys)) < 0.4, rng.choice(SPECIAL, len(keys)), rng.normal(size=len(keys))).astype(dt)
    return (keys // cols).astype(np.int32), (keys % cols).astype(np.int32), V


def _brute(a, b, cols, op, pattern, alpha, beta, dt):
    T = dt.type
    da = {int(i) * cols + int(j): T(v) for i, j, v in zip(*a)}
    db = {int(i) * cols + int(j): T(v) for i, j, v in zip(*b)}

    def sc(v, s):
        return v if s == 1.0 else T(T(s) * v)

    def f(x, y):
        if op == "plus":
            return T(x + y)
        if op == "times":
            return T(x * y)
        if op == "min":
            return y if math.isnan(x) else x if math.isnan(y) else min(x, y)
        if op == "max":
            return y if math.isnan(x) else x if math.isnan(y) else max(x, y)
        if op == "lor":
            return T(1) if (x != 0 or y != 0) else T(0)
        return T(1) if (x != 0 and y != 0) else T(0)

    keys = (da.keys() | db.keys()) if pattern == "union" else (da.keys() & db.keys())
    out = {}
    with np.errstate(all="ignore"):
        for k in keys:
            if k in da and k in db:
                out[k] = f(sc(da[k], alpha), sc(db[k], beta))
            elif k in da:
                out[k] = sc(da[k], alpha)
            else:
                out[k] = sc(db[k], beta)
    return out


def _same_value(x, y, op):
    if math.isnan(x) or math.isnan(y):
        return math.isnan(x) and math.isnan(y)
    if op in ("min", "max") and x == 0 and y == 0:
        return True    # (the sign of a zero result of fmin / fmax is not specified)
    return np.asarray(x).tobytes() == np.asarray(y).tobytes()


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
@pytest.mark.parametrize("pattern", er.PATTERNS)
@pytest.mark.parametrize("op", er.OPS)
def test_ewiseref_matches_brute_force(op, pattern, dtype):
    dt = np.dtype(dtype)
    rng = np.random.default_rng([er.OPS.index(op), er.PATTERNS.index(pattern), dt.itemsize])
    for rows, cols, na, nb in ((7, 9, 20, 25), (40, 33, 300, 200), (1, 50, 10, 40), (20, 20, 0, 30)):
        a = _operand(rng, rows, cols, na, dt)
        # B shares about half of A's positions
        bk = np.unique(np.concatenate([a[0].astype(np.int64) * cols + a[1], rng.choice(rows * cols, nb)])[: max(nb, 1)])
        bk = rng.permutation(bk)[:nb]
        bk.sort()
        b = ((bk // cols).astype(np.int32), (bk % cols).astype(np.int32),
             np.where(rng.random(len(bk)) < 0.4, rng.choice(SPECIAL, len(bk)), rng.normal(size=len(bk))).astype(dt))
        for alpha, beta in SCALES:
            I, J, V = er.ewise(cols, a, b, op, pattern, alpha, beta)
            assert V.dtype == dt
            want = _brute(a, b, cols, op, pattern, alpha, beta, dt)
            keys = I.astype(np.int64) * cols + J
            assert np.all(np.diff(keys) > 0), "result not canonical"
            assert sorted(want) == list(keys)
            for k, v in zip(keys, V):
                assert _same_value(v, want[int(k)], op), (op, pattern, alpha, beta, k, v, want[int(k)])


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
def test_unit_scales_copy_bits(dtype):
    """alpha = beta = 1: a value stored on one side only arrives bit for bit (NaN payloads, -0.0, subnormals)"""
    dt = np.dtype(dtype)
    ut = np.uint64 if dt == np.float64 else np.uint32
    bits = np.array([0x7FF8000000001234, 0x8000000000000000, 1, 0xFFF0000000000001], np.uint64) if dt == np.float64 else \
        np.array([0x7FC01234, 0x80000000, 1, 0xFF800001], np.uint32)
    V = bits.astype(ut).view(dt)
    a = (np.zeros(4, np.int32), np.arange(4, dtype=np.int32), V)
    b = (np.ones(1, np.int32), np.zeros(1, np.int32), np.array([5.0], dt))
    for op in er.OPS:
        I, J, R = er.ewise(4, a, b, op, "union")
        assert np.array_equal(R[:4].view(ut), bits.astype(ut))


def test_intersection_of_disjoint_is_empty():
    a = (np.array([0], np.int32), np.array([0], np.int32), np.array([1.0]))
    b = (np.array([1], np.int32), np.array([1], np.int32), np.array([2.0]))
    I, J, V = er.ewise(2, a, b, "plus", "intersect")
    assert len(I) == len(J) == len(V) == 0
    I, J, V = er.ewise(2, a, b, "plus", "union")
    assert list(I) == [0, 1] and list(V) == [1.0, 2.0]
