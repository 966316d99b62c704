"""CPU: the numpy reference of the sampled dense-dense product (sddmmref.py) against a naive per-entry loop (min / max / pair / lor)
and, for plus_times, against the dense oracle product X * Y^T sampled at the pattern -- a second, independent use of the oracle;
strided X / Y, X is Y, k = 0, the accumulate split property, and the argument checks of the four entry points that need no device."""
import ctypes as C
import math

import numpy as np
import pytest

import sddmmref as sd
import semiringref as sr
from matgen import cases

CASES = cases()
NAMES = ("tiny_9x9", "rand_50", "rect_70x40_AAt", "empty_rows", "cancel_and_zero", "empty_matrix")
PEM_E_INVALID = -1
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3.0e-310, 1.0e-40, 0.5, -0.5])
MINMAX = ("min_plus", "max_plus", "max_times")
DTYPES = (np.float64, np.float32)


def _same(got, want, kind="plus_times"):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    ok = (got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want))
    if kind in MINMAX:
        ok |= (got == 0) & (want == 0)
    return bool(np.all(ok))


def _block(n, ld, seed, dtype):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, ld))
    sp = rng.random((n, ld)) < 0.25
    B[sp] = rng.choice(SPECIAL, int(sp.sum()))
    return B.astype(dtype)


def _pattern(name):
    rows, cols, I, J, V, _ = CASES[name]
    rp, ci, _ = sr.coo_to_csr(rows, cols, I, J, np.asarray(V, np.float64))
    return (rows, cols) + sd.pattern_of(rows, rp, ci)


def _naive(I, J, X, Y, s, dtype, old=None):
    """one entry at a time, one column at a time, scalars of the value type"""
    t = np.dtype(dtype).type
    out = np.zeros(len(I), dtype)
    with np.errstate(all="ignore"):
        for e, (i, j) in enumerate(zip(I, J)):
            if old is None:
                acc = t(sd.START[s])
            else:
                acc = t(old[e] != 0) if s == "lor_land" else t(old[e])
            for c in range(X.shape[1]):
                x, y = t(X[i, c]), t(Y[j, c])
                if s == "plus_pair":
                    acc = t(acc + t(1))
                elif s == "lor_land":
                    acc = t(1) if (x != 0 and y != 0) else acc
                else:
                    term = t(x + y) if s in ("min_plus", "max_plus") else t(x * y)
                    if not math.isnan(term):
                        if math.isnan(acc):
                            acc = term
                        elif s == "min_plus":
                            acc = term if term < acc else acc
                        else:
                            acc = term if term > acc else acc
            out[e] = acc
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", NAMES)
def test_folds_against_a_naive_loop(name, dtype):
    rows, cols, I, J = _pattern(name)
    k = 5
    X, Y = _block(rows, 7, 1, dtype)[:, :k], _block(cols, 9, 2, dtype)[:, 2:2 + k]   # column slices: row strides 7 and 9
    old = _block(len(I), 1, 3, dtype)[:, 0]
    for s in ("min_plus", "max_plus", "max_times", "plus_pair", "lor_land"):
        for o in (None, old):
            assert _same(sd.sddmm(I, J, X, Y, s, dtype, old=o), _naive(I, J, X, Y, s, dtype, old=o), s), f"{name} {s} accumulate={o is not None}"


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", NAMES)
def test_plus_times_against_the_dense_oracle_product(oracle, name, dtype):
    """X * Y^T as the oracle's product of two dense matrices (every element stored), sampled at the pattern.  Finite values: a dense
    product meets every chain alike, so this needs no special values to tell the chains apart."""
    rows, cols, I, J = _pattern(name)
    k = 6
    rng = np.random.default_rng(7)
    X, Y = rng.standard_normal((rows, k + 2)).astype(dtype)[:, 1:1 + k], rng.standard_normal((cols, k)).astype(dtype)
    X[rng.random(X.shape) < 0.2] = 0
    ii, cc = np.meshgrid(np.arange(rows), np.arange(k), indexing="ij")
    jj, c2 = np.meshgrid(np.arange(cols), np.arange(k), indexing="ij")
    A = oracle.Csr(rows, k, ii.ravel(), cc.ravel(), np.asarray(X, np.float64).ravel())
    B = oracle.Csr(k, cols, c2.ravel(), jj.ravel(), np.asarray(Y, np.float64).ravel())
    crp, cci, cv = oracle.csr_spgemm(A, B, f32=np.dtype(dtype) == np.float32).arrays()
    assert np.all(np.diff(crp) == cols)
    D = np.asarray(cv).astype(dtype).reshape(rows, cols)
    assert _same(sd.sddmm(I, J, X, Y, "plus_times", dtype, oracle=oracle), D[I, J])


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_x_is_y_and_zero_columns(oracle, dtype):
    rows, cols, I, J = _pattern("rand_50")
    H = _block(rows, 4, 5, dtype)
    for s in sd.SEMIRINGS:
        assert _same(sd.sddmm(I, J, H, H, s, dtype, oracle=oracle), sd.sddmm(I, J, H, H.copy(), s, dtype, oracle=oracle), s)
        got = sd.sddmm(I, J, H[:, :0], H[:, :0], s, dtype, oracle=oracle)
        assert _same(got, np.full(len(I), sd.START[s], dtype)), f"{s}: k = 0 stores the start value"
    old = _block(len(I), 1, 6, dtype)[:, 0]
    assert _same(sd.sddmm(I, J, H[:, :0], H[:, :0], "plus_times", dtype, old=old, oracle=oracle), old)
    assert _same(sd.sddmm(I, J, H[:, :0], H[:, :0], "lor_land", dtype, old=old), (old != 0).astype(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", ("rand_50", "rect_70x40_AAt", "cancel_and_zero"))
def test_accumulate_splits_the_columns(oracle, name, dtype):
    """one call with k = k1 + k2 equals a call on [0, k1) followed by an accumulate call on [k1, k1 + k2)"""
    rows, cols, I, J = _pattern(name)
    k1, k2 = 3, 4
    X, Y = _block(rows, k1 + k2, 8, dtype), _block(cols, k1 + k2, 9, dtype)
    for s in sd.SEMIRINGS:
        whole = sd.sddmm(I, J, X, Y, s, dtype, oracle=oracle)
        first = sd.sddmm(I, J, X[:, :k1], Y[:, :k1], s, dtype, oracle=oracle)
        both = sd.sddmm(I, J, X[:, k1:], Y[:, k1:], s, dtype, old=first, oracle=oracle)
        assert _same(both, whole, s), f"{name} {s}"


def test_null_context_is_refused(pkg):
    L = pkg.lib()
    i64 = C.c_int64
    for fn in (L.pem_tiled_set_values_sddmm, L.pem_tiled_set_values_sddmm_f32):
        assert fn(None, None, 0, i64(1), None, i64(1), None, i64(1), 0) == PEM_E_INVALID
        assert b"null context" in L.pem_last_error() and b"pem_tiled_set_values_sddmm" in L.pem_last_error()
    for fn in (L.pem_tiled_sddmm, L.pem_tiled_sddmm_f32):
        out = C.c_void_p()
        assert fn(None, None, 0, i64(1), None, i64(1), None, i64(1), C.byref(out)) == PEM_E_INVALID
        assert b"null context" in L.pem_last_error() and b"pem_tiled_sddmm" in L.pem_last_error()
