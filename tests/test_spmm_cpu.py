"""CPU: the numpy reference of the sparse-times-dense-block products (spmmref.py) against mxvref column by column, with strided X and
Y and accumulate, and the argument checks of pem_tiled_spmm / pem_tiled_spmm_f32 that need no device."""
import ctypes as C

import numpy as np
import pytest

import mxvref as mr
import semiringref as sr
import spmmref as spr
from matgen import cases

CASES = cases()
PEM_E_INVALID = -1
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3.0e-310, 1.0e-40, 0.5, -0.5])


def _same(got, want, zero_sign=True):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    ok = (got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want))
    if not zero_sign:
        ok |= (got == 0) & (want == 0)
    return bool(np.all(ok))


def _block(n, ld, seed, dtype):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, ld))
    sp = rng.random((n, ld)) < 0.25
    B[sp] = rng.choice(SPECIAL, int(sp.sum()))
    return B.astype(dtype)


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
@pytest.mark.parametrize("transpose", (False, True))
@pytest.mark.parametrize("name", ("tiny_9x9", "rand_50", "rect_70x40_AAt", "empty_rows", "cancel_and_zero", "empty_matrix"))
def test_reference_is_mxvref_per_column(oracle, name, transpose, dtype):
    rows, cols, I, J, V, _ = CASES[name]
    rp, ci, v = sr.coo_to_csr(rows, cols, I, J, np.asarray(V, np.float64).astype(dtype))
    nx, ny = (rows, cols) if transpose else (cols, rows)
    k, ldx, ldy = 5, 7, 9
    X = _block(nx, ldx, 1, dtype)[:, :k]   # a column slice: row stride 7
    Yfull = _block(ny, ldy, 2, dtype)
    for s in mr.SEMIRINGS:
        for acc in (False, True):
            got = spr.spmm_into(rows, cols, rp, ci, v, X, Yfull, k, s, dtype, accumulate=acc, oracle=oracle, transpose=transpose)
            assert _same(got[:, k:], Yfull[:, k:]), f"{name} {s}: the padding columns changed"
            for c in range(k):
                y0 = Yfull[:, c].copy() if acc else None
                want = mr.mxv(rows, cols, rp, ci, v, X[:, c].copy(), s, dtype, y0=y0, oracle=oracle, transpose=transpose)
                assert _same(got[:, c], want), f"{name} {s} accumulate={acc} column {c}"


def test_zero_columns(oracle):
    rows, cols, I, J, V, _ = CASES["rand_50"]
    rp, ci, v = sr.coo_to_csr(rows, cols, I, J, np.asarray(V, np.float64))
    Y = spr.spmm(rows, cols, rp, ci, v, np.zeros((cols, 0)), "plus_times", np.float64, oracle=oracle)
    assert Y.shape == (rows, 0)


def test_null_context_is_refused(pkg):
    L = pkg.lib()
    for fn in (L.pem_tiled_spmm, L.pem_tiled_spmm_f32):
        assert fn(None, None, 0, 0, C.c_int64(1), None, C.c_int64(1), None, C.c_int64(1), 0) == PEM_E_INVALID
        assert b"null context" in L.pem_last_error()
