"""CPU: assignref (the numpy restatement of pem_tiled_assign) against a per-entry dictionary brute force and, densely, against scipy's
C[I][:, J] = A; the list rule; the package exposes the methods and the library exports the symbols."""
import numpy as np
import pytest
import scipy.sparse as sp

import assignref as ar
import ewiseref as ew

DTYPES = (np.float64, np.float32)
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3.0e-310, 1.0e-40, 0.5, -0.5])
SHAPES = ((23, 31, 160), (1, 40, 17), (40, 1, 17), (37, 37, 0), (16, 16, 256), (50, 20, 300))
ACCUMS = (None, "plus", "min")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _matrix(seed, rows, cols, nnz, dtype, special=True):
    rng = np.random.default_rng(seed)
    key = np.sort(rng.choice(rows * cols, min(nnz, rows * cols), replace=False)) if nnz else np.zeros(0, np.int64)
    V = rng.normal(size=len(key))
    if special:
        s = rng.random(len(key)) < 0.3
        V[s] = rng.choice(SPECIAL, int(s.sum()))
    return (key // cols).astype(np.int32), (key % cols).astype(np.int32), V.astype(dtype)


def _lists(rng, dim):
    """the kinds of list of the issue: null, range, permutation, half permutation, single, reversed"""
    return {"none": None, "range": np.arange(dim // 3, max(dim // 3 + 1, dim - dim // 4)), "perm": rng.permutation(dim),
            "half_perm": rng.permutation(dim)[: max(1, dim // 2)], "single": np.array([dim // 2]), "reversed": np.arange(dim)[::-1]}


def _brute(cols, C, A, RI, CJ, accum, rows):
    """one dictionary entry at a time"""
    RI = list(range(rows)) if RI is None else [int(x) for x in RI]
    CJ = list(range(cols)) if CJ is None else [int(x) for x in CJ]
    z = {(int(i), int(j)): v for i, j, v in zip(*C)}
    if accum is None:
        rs, cs = set(RI), set(CJ)
        for k in [k for k in z if k[0] in rs and k[1] in cs]:
            del z[k]
    for p, q, v in zip(*A):
        k = (RI[int(p)], CJ[int(q)])
        z[k] = ew.apply_op(accum, np.array([z[k]], C[2].dtype), np.array([v], C[2].dtype))[0] if k in z else v
    keys = sorted(z)
    return (np.array([k[0] for k in keys], np.int32), np.array([k[1] for k in keys], np.int32),
            np.array([z[k] for k in keys], C[2].dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_%d" % s)
def test_assignref_equals_brute_force(shape, dtype):
    rows, cols, nnz = shape
    C = _matrix(rows * 100 + cols, rows, cols, nnz, dtype)
    rng = np.random.default_rng(nnz + rows)
    rl, cl = _lists(rng, rows), _lists(rng, cols)
    for rn, RI in rl.items():
        for cn, CJ in cl.items():
            ni, nj = rows if RI is None else len(RI), cols if CJ is None else len(CJ)
            for fill in (0, (ni * nj + 2) // 3, ni * nj):
                A = _matrix(ni * 7 + nj + fill, ni, nj, fill, dtype)
                for accum in ACCUMS:
                    got = ar.assign(rows, cols, C, A, RI, CJ, accum)
                    want = _brute(cols, C, A, RI, CJ, accum, rows)
                    assert got[2].dtype == np.dtype(dtype)
                    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (rn, cn, fill, accum)
                    if accum == "min":                    # (fmin leaves the sign of a zero result free)
                        same = (_bits(got[2]) == _bits(want[2])) | ((got[2] == 0) & (want[2] == 0)) | (np.isnan(got[2]) & np.isnan(want[2]))
                    elif accum == "plus":                 # (a NaN that arithmetic produces has an unspecified payload)
                        same = (_bits(got[2]) == _bits(want[2])) | (np.isnan(got[2]) & np.isnan(want[2]))
                    else:
                        same = _bits(got[2]) == _bits(want[2])
                    assert bool(np.all(same)), (rn, cn, fill, accum)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_%d" % s)
def test_assignref_equals_scipy_densely(shape):
    """scipy's sparse __setitem__ keeps zeroed entries stored, so only the dense values are compared (finite values)"""
    rows, cols, nnz = shape
    C = _matrix(rows * 100 + cols, rows, cols, nnz, np.float64, special=False)
    rng = np.random.default_rng(nnz + rows + 1)
    rl, cl = _lists(rng, rows), _lists(rng, cols)
    Cd = sp.csr_matrix((C[2], (C[0], C[1])), shape=(rows, cols)).toarray()
    for rn, RI in rl.items():
        for cn, CJ in cl.items():
            ni, nj = rows if RI is None else len(RI), cols if CJ is None else len(CJ)
            A = _matrix(ni * 7 + nj, ni, nj, (ni * nj + 2) // 3, np.float64, special=False)
            Ad = sp.csr_matrix((A[2], (A[0], A[1])), shape=(ni, nj)).toarray()
            ix = np.ix_(np.arange(rows) if RI is None else RI, np.arange(cols) if CJ is None else CJ)
            for accum in (None, "plus"):
                want = Cd.copy()
                want[ix] = Ad if accum is None else want[ix] + Ad
                zi, zj, zv = ar.assign(rows, cols, C, A, RI, CJ, accum)
                got = np.zeros((rows, cols))
                got[zi, zj] = zv
                assert np.array_equal(got, want), (rn, cn, accum)


def test_lists_are_checked():
    for bad in ([], [-1], [5], [0.5], [[0]], [1, 1], [0, 3, 2, 3]):
        with pytest.raises(ValueError):
            ar.check_list(np.array(bad), 5)
    assert np.array_equal(ar.check_list([4, 0, 2], 5), [4, 0, 2])
    one = ([0], [0], np.array([1.0]))
    with pytest.raises(ValueError):
        ar.assign(5, 5, one, one, RI=[5], CJ=[0])
    with pytest.raises(ValueError):
        ar.assign(5, 5, one, one, RI=[0], CJ=[-1])
    with pytest.raises(ValueError):
        ar.assign(5, 5, one, ([0, 1], [0, 0], np.array([1.0, 2.0])), RI=[2, 2], CJ=[0])
    with pytest.raises(ValueError):
        ar.assign(5, 5, one, ([1], [0], np.array([1.0])), RI=[2], CJ=[0])   # A does not fit 1 x 1


def test_package_has_the_methods_and_library_exports_the_symbols(pkg):
    for m in ("assign", "set_values_from_assign"):
        assert callable(getattr(pkg.Tiled, m, None)), f"Tiled.{m} is missing"
    for sym in ("pem_tiled_assign", "pem_tiled_assign_device", "pem_tiled_set_values_from_assign"):
        assert sym in pkg.ABI_SYMBOLS
        assert hasattr(pkg.lib(), sym), f"the library does not export {sym}"
