"""CPU: extractref (the numpy restatement of pem_tiled_extract / pem_tiled_transpose) against a per-entry brute force and against
scipy's A[I][:, J]; the package exposes the methods and the library exports the symbols."""
import numpy as np
import pytest
import scipy.sparse as sp

import extractref as ex

DTYPES = (np.float64, np.float32)
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3.0e-310, 1.0e-40, 0.5, -0.5])


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _matrix(seed, rows, cols, nnz, dtype):
    rng = np.random.default_rng(seed)
    key = np.sort(rng.choice(rows * cols, min(nnz, rows * cols), replace=False)) if nnz else np.zeros(0, np.int64)
    V = rng.normal(size=len(key))
    s = rng.random(len(key)) < 0.3
    V[s] = rng.choice(SPECIAL, int(s.sum()))
    return (key // cols).astype(np.int32), (key % cols).astype(np.int32), V.astype(dtype)


def _lists(rng, dim, I_used):
    """the kinds of list of the issue: identity, ranges, reversed, permutation, with repeats, single-element, only empty"""
    out = {"none": None, "identity": np.arange(dim), "range": np.arange(dim // 3, max(dim // 3 + 1, dim - dim // 4)),
           "reversed": np.arange(dim)[::-1], "perm": rng.permutation(dim), "repeats": rng.integers(0, dim, 2 * dim + 3),
           "single": np.array([dim // 2]), "one_x5": np.full(5, dim - 1)}
    empty = np.setdiff1d(np.arange(dim), I_used)
    if len(empty):
        out["empty_only"] = np.concatenate([empty, empty[:2]])
    return out


def _brute(rows, cols, I, J, V, RI, CJ):
    at = {(int(i), int(j)): k for k, (i, j) in enumerate(zip(I, J))}
    RI = range(rows) if RI is None else RI
    CJ = range(cols) if CJ is None else CJ
    oi, oj, ok = [], [], []
    for p, i in enumerate(RI):
        for q, j in enumerate(CJ):
            k = at.get((int(i), int(j)))
            if k is not None:
                oi.append(p), oj.append(q), ok.append(k)
    return np.array(oi, np.int32), np.array(oj, np.int32), np.asarray(V)[np.array(ok, np.int64)]


SHAPES = ((23, 31, 160), (1, 40, 17), (40, 1, 17), (37, 37, 0), (16, 16, 256), (50, 20, 300))


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_%d" % s)
def test_extractref_equals_brute_force_and_scipy(shape, dtype):
    rows, cols, nnz = shape
    I, J, V = _matrix(rows * 100 + cols, rows, cols, nnz, dtype)
    rng = np.random.default_rng(nnz + rows)
    S = sp.csr_matrix((V, (I, J)), shape=(rows, cols))
    assert S.nnz == len(V)                                # (explicit zeros are kept by the constructor)
    rl, cl = _lists(rng, rows, I), _lists(rng, cols, J)
    for rn, RI in rl.items():
        for cn, CJ in cl.items():
            ni, nj, oi, oj, ov = ex.extract(rows, cols, I, J, V, RI, CJ)
            assert (ni, nj) == (rows if RI is None else len(RI), cols if CJ is None else len(CJ))
            assert ov.dtype == np.dtype(dtype)
            bi, bj, bv = _brute(rows, cols, I, J, V, RI, CJ)
            assert np.array_equal(oi, bi) and np.array_equal(oj, bj), (rn, cn)
            assert np.array_equal(_bits(ov), _bits(bv)), (rn, cn)
            X = S
            if RI is not None:
                X = X[RI]
            if CJ is not None:
                X = X[:, CJ]
            X = sp.csr_matrix(X)
            X.sort_indices()
            assert X.shape == (ni, nj) and X.nnz == len(ov), (rn, cn)
            assert np.array_equal(np.repeat(np.arange(ni), np.diff(X.indptr)), oi) and np.array_equal(X.indices, oj), (rn, cn)
            assert np.array_equal(_bits(X.data.astype(dtype)), _bits(ov)), (rn, cn)


def test_transpose_ref():
    I, J, V = _matrix(5, 23, 31, 160, np.float64)
    r, c, ti, tj, tv = ex.transpose(23, 31, I, J, V)
    assert (r, c) == (31, 23)
    T = sp.csr_matrix((V, (I, J)), shape=(23, 31)).T.tocsr()
    T.sort_indices()
    assert np.array_equal(np.repeat(np.arange(31), np.diff(T.indptr)), ti) and np.array_equal(T.indices, tj)
    assert np.array_equal(_bits(T.data), _bits(tv))
    back = ex.transpose(r, c, ti, tj, tv)
    assert np.array_equal(back[2], I) and np.array_equal(back[3], J) and np.array_equal(_bits(back[4]), _bits(V))


def test_selection_matrices_give_the_extract():
    """the device route of the cross-check: P*A*Q with P[p, I[p]] = 1 and Q[J[q], q] = 1 is A(I, J)"""
    I, J, V = _matrix(8, 30, 20, 150, np.float64)
    V = np.where(np.isfinite(V), V, 1.5)
    rng = np.random.default_rng(2)
    RI, CJ = rng.integers(0, 30, 41), rng.integers(0, 20, 33)
    A = sp.csr_matrix((V, (I, J)), shape=(30, 20))
    pr, pc, pi, pj, pv = ex.selection(41, 30, RI, left=True)
    qr, qc, qi, qj, qv = ex.selection(33, 20, CJ, left=False)
    P, Q = sp.csr_matrix((pv, (pi, pj)), shape=(pr, pc)), sp.csr_matrix((qv, (qi, qj)), shape=(qr, qc))
    ni, nj, oi, oj, ov = ex.extract(30, 20, I, J, V, RI, CJ)
    D = np.zeros((ni, nj))
    D[oi, oj] = ov
    assert np.array_equal((P @ A @ Q).toarray(), D)


def test_lists_are_checked():
    for bad in ([], [-1], [5], [0.5], [[0]]):
        with pytest.raises(ValueError):
            ex.check_list(np.array(bad), 5)
    with pytest.raises(ValueError):
        ex.extract(5, 5, [0], [0], [1.0], RI=[5])
    with pytest.raises(ValueError):
        ex.extract(5, 5, [0], [0], [1.0], CJ=[-1])


def test_package_has_the_methods_and_library_exports_the_symbols(pkg):
    for m in ("extract", "transpose", "set_values_from_extract", "set_values_from_transpose"):
        assert callable(getattr(pkg.Tiled, m, None)), f"Tiled.{m} is missing"
    for sym in ("pem_tiled_transpose", "pem_tiled_set_values_from_transpose", "pem_tiled_extract", "pem_tiled_extract_device",
                "pem_tiled_set_values_from_extract"):
        assert sym in pkg.ABI_SYMBOLS
        assert hasattr(pkg.lib(), sym), f"the library does not export {sym}"
