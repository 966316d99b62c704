"""CPU: tests/kronref.py against independent statements -- np.kron of the dense forms, the transpose rule, the mixed-product identity
through the oracle's serial CSR product, a direct double loop for the other ops -- and the library's exports, the header's
declarations and the package's op table."""
import os
import re

import numpy as np
import pytest

import kronref

DTYPES = (np.float64, np.float32)
IDS = ("f64", "f32")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pem_spgemm.h")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _sparse(rng, rows, cols, n, dt, integers=False):
    """canonical (I, J, V) with non-zero values"""
    keys = np.sort(rng.choice(rows * cols, size=min(n, rows * cols), replace=False))
    V = rng.integers(1, 6, len(keys)) * rng.choice([-1, 1], len(keys)) if integers else rng.normal(size=len(keys))
    V = np.asarray(V, dt)
    V[V == 0] = 1
    return (keys // cols).astype(np.int32), (keys % cols).astype(np.int32), V


def _dense(rows, cols, I, J, V):
    D = np.zeros((rows, cols), V.dtype)
    D[I, J] = V
    return D


SHAPES = (((12, 9, 40), (7, 5, 12)), ((1, 1, 1), (7, 5, 35)), ((5, 4, 20), (1, 1, 1)), ((3, 3, 5), (3, 3, 5)), ((1, 9, 4), (6, 1, 3)),
          ((4, 4, 0), (3, 2, 4)))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_times_equals_numpys_kron_of_the_dense_forms(dtype):
    rng = np.random.default_rng(1)
    for (ra, ca, na), (rb, cb, nb) in SHAPES:
        IA, JA, VA = _sparse(rng, ra, ca, na, dtype)
        IB, JB, VB = _sparse(rng, rb, cb, nb, dtype)
        rows, cols, I, J, V = kronref.kron(ra, ca, IA, JA, VA, rb, cb, IB, JB, VB, "times", dtype)
        assert (rows, cols) == (ra * rb, ca * cb) and V.dtype == np.dtype(dtype) and I.dtype == J.dtype == np.int32
        assert len(I) == len(IA) * len(IB)
        key = I.astype(np.int64) * cols + J
        assert np.all(np.diff(key) > 0), "canonical: sorted, no duplicates"
        DA, DB = _dense(ra, ca, IA, JA, VA), _dense(rb, cb, IB, JB, VB)
        want = np.kron(DA, DB)
        assert want.dtype == np.dtype(dtype)
        pattern = np.kron(DA != 0, DB != 0)                      # where both operands are non-zero
        got_pattern = np.zeros((rows, cols), bool)
        got_pattern[I, J] = True
        assert np.array_equal(got_pattern, pattern)
        assert np.array_equal(_bits(V), _bits(want[I, J]))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_transpose_rule(dtype):
    rng = np.random.default_rng(2)
    for (ra, ca, na), (rb, cb, nb) in SHAPES:
        IA, JA, VA = _sparse(rng, ra, ca, na, dtype)
        IB, JB, VB = _sparse(rng, rb, cb, nb, dtype)
        for op in kronref.BINOPS:
            rows, cols, I, J, V = kronref.kron(ra, ca, IA, JA, VA, rb, cb, IB, JB, VB, op, dtype)
            tr, tc, tI, tJ, tV = kronref.kron(ca, ra, JA, IA, VA, cb, rb, JB, IB, VB, op, dtype)
            assert (tr, tc) == (cols, rows)
            o = np.lexsort((I, J))                               # the transpose of the first, made canonical
            assert np.array_equal(J[o], tI) and np.array_equal(I[o], tJ) and np.array_equal(_bits(V[o]), _bits(tV))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_mixed_product_identity_through_the_oracle(oracle, dtype):
    """(A (x) B)(C (x) D) = AC (x) BD on integer-valued matrices: every product and sum is exact, so the two sides agree exactly --
    in the pattern too: an entry of either side is a sum over pairs (x, y) that factors into AC's and BD's sums."""
    f32 = dtype == np.float32
    rng = np.random.default_rng(3)
    for (m, n, p), (r, s, t) in (((5, 4, 6), (3, 7, 2)), ((1, 6, 3), (4, 1, 5)), ((9, 9, 9), (2, 2, 2))):
        A, Cm = _sparse(rng, m, n, 11, dtype, True), _sparse(rng, n, p, 9, dtype, True)
        B, D = _sparse(rng, r, s, 8, dtype, True), _sparse(rng, s, t, 6, dtype, True)
        csr = lambda rows, cols, I, J, V: oracle.Csr(rows, cols, I, J, np.asarray(V, np.float64))
        AB = kronref.kron(m, n, *A, r, s, *B, "times", dtype)
        CD = kronref.kron(n, p, *Cm, s, t, *D, "times", dtype)
        lp, lj, lv = oracle.csr_spgemm(csr(*AB), csr(*CD), f32=f32).arrays()
        ap_, aj, av = oracle.csr_spgemm(csr(m, n, *A), csr(n, p, *Cm), f32=f32).arrays()
        bp, bj, bv = oracle.csr_spgemm(csr(r, s, *B), csr(s, t, *D), f32=f32).arrays()
        aI, bI = np.repeat(np.arange(m), np.diff(ap_)), np.repeat(np.arange(r), np.diff(bp))
        rows, cols, I, J, V = kronref.kron(m, p, aI, aj, np.asarray(av, dtype), r, t, bI, bj, np.asarray(bv, dtype), "times", dtype)
        lI = np.repeat(np.arange(m * r), np.diff(lp))
        # pattern and values, cancelled zeros included: both sides store (i r, p t) where some x and some y give a path (a product of
        # sums may be -0 where the sum of products is +0: compared as numbers)
        assert np.array_equal(lI, I) and np.array_equal(lj, J)
        assert np.array_equal(np.asarray(lv, dtype), V) and np.count_nonzero(V) > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_every_op_against_a_double_loop(dtype):
    dt = np.dtype(dtype)
    rng = np.random.default_rng(4)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 0.5, -2.0], dt)
    ra, ca, rb, cb = 4, 5, 3, 2
    IA, JA, _ = _sparse(rng, ra, ca, 9, dtype)
    IB, JB, _ = _sparse(rng, rb, cb, 5, dtype)
    VA, VB = rng.choice(special, len(IA)), rng.choice(special, len(IB))
    scalar = dict(plus=lambda a, b: a + b, times=lambda a, b: a * b, min=np.fmin, max=np.fmax,
                  lor=lambda a, b: dt.type((a != 0) or (b != 0)), land=lambda a, b: dt.type((a != 0) and (b != 0)))
    for op in kronref.BINOPS:
        rows, cols, I, J, V = kronref.kron(ra, ca, IA, JA, VA, rb, cb, IB, JB, VB, op, dtype)
        want = {}
        with np.errstate(all="ignore"):
            for x in range(len(IA)):
                for y in range(len(IB)):
                    want[(int(IA[x]) * rb + int(IB[y]), int(JA[x]) * cb + int(JB[y]))] = dt.type(scalar[op](VA[x], VB[y]))
        assert len(want) == len(I) == len(IA) * len(IB)
        for i, j, v in zip(I, J, V):
            w = want[(int(i), int(j))]
            assert (np.isnan(v) and np.isnan(w)) or v.tobytes() == w.tobytes() or (op in ("min", "max") and v == w == 0), (op, i, j, v, w)
    with pytest.raises(ValueError):
        kronref.kron(ra, ca, IA, JA, VA, rb, cb, IB, JB, VB, "minus", dtype)
    with pytest.raises(OverflowError):
        kronref.kron(65536, 1, [0], [0], VA[:1], 65536, 1, [0], [0], VB[:1])


def test_library_exports_header_declares_and_package_lists_the_ops(pkg):
    for sym in ("pem_tiled_kron", "pem_tiled_set_values_from_kron"):
        assert sym in pkg.ABI_SYMBOLS
        assert hasattr(pkg.lib(), sym), f"the library does not export {sym}"
    text = open(HEADER).read()
    assert re.search(r"pem_status\s+pem_tiled_kron\(pem_ctx \*ctx, const pem_tiled \*A, const pem_tiled \*B, int op, pem_tiled \*\*out\);", text)
    assert re.search(r"pem_status\s+pem_tiled_set_values_from_kron\(pem_ctx \*ctx, pem_tiled \*t, const pem_tiled \*A, const pem_tiled \*B\);", text)
    # the Python op table is the pem_binop enum
    enum = re.search(r"typedef enum \{([^}]*)\} pem_binop;", text).group(1)
    table = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"PEM_BINOP_(\w+)\s*=\s*(\d+)", enum)}
    assert table == pkg.BINOPS
    assert tuple(sorted(pkg.BINOPS, key=pkg.BINOPS.get)) == kronref.BINOPS
    assert callable(pkg.Tiled.kron) and callable(pkg.Tiled.set_values_from_kron)
