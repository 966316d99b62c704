"""CPU: tests/semiringref.py (the numpy statement of the six semirings) against a dense brute force."""
import numpy as np
import pytest

import semiringref as sr
from matgen import random_coo

with np.errstate(invalid="ignore"):
    SPECIAL = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.5, -2.0, 3.25, 1e308, -1e308, 5e-324])


def _csr_to_dense(rp, ci, v, rows, cols, dtype):
    present = np.zeros((rows, cols), bool)
    val = np.zeros((rows, cols), dtype)
    r = np.repeat(np.arange(rows), np.diff(rp))
    present[r, ci] = True
    val[r, ci] = v
    return present, val


def _check(rows, inner, cols, A, B, semiring, dtype, chunk=1 << 22):
    ca = sr.coo_to_csr(rows, inner, *A)
    cb = sr.coo_to_csr(inner, cols, *B)
    rp, ci, v = sr.spgemm(ca, cb, cols, semiring, dtype, chunk=chunk)
    assert v.dtype == np.dtype(dtype)
    assert np.all(np.diff(rp) >= 0) and rp[-1] == len(ci)
    for r in range(rows):                                          # columns ascend inside a row
        assert np.all(np.diff(ci[rp[r]:rp[r + 1]]) > 0)
    present, val = _csr_to_dense(rp, ci, v, rows, cols, dtype)
    wp, wv = sr.dense(rows, inner, *A, semiring, dtype, B=(inner, cols, *B))
    assert np.array_equal(present, wp)
    if semiring == "plus_times":
        with np.errstate(invalid="ignore"):
            assert np.allclose(val[wp], wv[wp], rtol=1e-5 if dtype == np.float32 else 1e-12, equal_nan=True)
    else:
        assert sr.same_values(val[wp], wv[wp])
    return rp, ci, v


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("semiring", sr.SEMIRINGS)
def test_random_against_dense(semiring, dtype):
    rng = np.random.default_rng(3)
    for rows, inner, cols, na, nb in ((12, 9, 14, 40, 50), (20, 20, 20, 90, 90), (1, 30, 5, 10, 40), (25, 7, 3, 60, 15), (18, 10, 10, 8, 30)):
        A = random_coo(rng, rows, inner, na)[2:]
        B = random_coo(rng, inner, cols, nb)[2:]
        _check(rows, inner, cols, A, B, semiring, dtype)
        _check(rows, inner, cols, A, B, semiring, dtype, chunk=7)      # many row blocks, one row at least per block


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("semiring", sr.SEMIRINGS)
def test_special_values_against_dense(semiring, dtype):
    rng = np.random.default_rng(8)
    rows, inner, cols = 10, 12, 11
    _, _, I, J, _ = random_coo(rng, rows, inner, 70)
    _, _, K, L, _ = random_coo(rng, inner, cols, 70)
    A = (I, J, rng.choice(SPECIAL, len(I)))
    B = (K, L, rng.choice(SPECIAL, len(K)))
    with np.errstate(all="ignore"):
        _check(rows, inner, cols, A, B, semiring, dtype)


def test_rules():
    """the spelled-out rules on hand-made entries"""
    with np.errstate(all="ignore"):
        # C(0,0): products over k = 0, 1, 2;  C(0,1): one NaN product only
        A = (np.array([0, 0, 0]), np.array([0, 1, 2]), np.array([np.nan, 2.0, -1.0]))
        B = (np.array([0, 1, 2, 0]), np.array([0, 0, 0, 1]), np.array([1.0, 0.0, 4.0, 5.0]))
        ca, cb = sr.coo_to_csr(1, 3, *A), sr.coo_to_csr(3, 2, *B)
        get = lambda s: sr.spgemm(ca, cb, 2, s)[2]
        assert list(get("min_plus")) == [2.0, np.inf]                  # (nan+1) skipped; min(2+0, -1+4); all-NaN -> +inf
        assert list(get("max_plus")) == [3.0, -np.inf]
        assert list(get("max_times")) == [0.0, -np.inf]                # max(2*0, -1*4)
        assert list(get("plus_pair")) == [3.0, 1.0]                    # NaN values count like any other
        assert list(get("lor_land")) == [1.0, 1.0]                     # (nan, 1): NaN != 0;  (2, 0): no;  (-1, 4): yes
        B0 = (B[0], B[1], np.array([0.0, 0.0, 0.0, 0.0]))
        assert list(sr.spgemm(ca, sr.coo_to_csr(3, 2, *B0), 2, "lor_land")[2]) == [0.0, 0.0]   # entries stay, value 0
    # per-product rounding in fp32: 1 + 2^-30 rounds to 1 in float32
    ca = sr.coo_to_csr(1, 1, [0], [0], [1.0])
    cb = sr.coo_to_csr(1, 1, [0], [0], [2.0 ** -30])
    assert sr.spgemm(ca, cb, 1, "min_plus", np.float32)[2][0] == np.float32(1.0)
    assert sr.spgemm(ca, cb, 1, "min_plus", np.float64)[2][0] == 1.0 + 2.0 ** -30


def test_filter_and_transpose():
    rng = np.random.default_rng(5)
    rows, cols, I, J, V = random_coo(rng, 30, 20, 120)
    rp, ci, v = sr.coo_to_csr(rows, cols, I, J, V)
    trp, tci, tv = sr.transpose_csr(rows, cols, rp, ci, v)
    D = np.zeros((rows, cols))
    D[I, J] = V
    pt, vt = _csr_to_dense(trp, tci, tv, cols, rows, np.float64)
    assert np.array_equal(vt, D.T) and pt.sum() == len(I)
    MI, MJ = I[::3], J[::3]
    frp, fci, fv = sr.filter_csr(rp, ci, v, cols, MI, MJ)
    crp, cci, cv = sr.filter_csr(rp, ci, v, cols, MI, MJ, complement=True)
    assert frp[-1] + crp[-1] == len(ci) and frp[-1] == len(MI)
    assert sorted(fv.tolist() + cv.tolist()) == sorted(v.tolist())
