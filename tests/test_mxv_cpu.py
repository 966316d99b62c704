"""CPU: the numpy reference of the matrix-vector products and reductions (mxvref.py) against the oracle and against independent
statements of the same folds -- the yardstick the GPU tests of pem_tiled_mxv / pem_tiled_reduce use."""
from fractions import Fraction

import numpy as np
import pytest

import mxvref as mr
import semiringref as sr
from matgen import cases

CASES = cases()
SMALL = ("tiny_9x9", "one_entry", "rand_50", "rand_300", "rect_70x40_AAt", "rect_33x65_AAt", "ragged_37", "dense_48", "empty_rows",
         "empty_matrix", "row_vector_AAt", "col_vector_AAt", "cancel_and_zero", "powerlaw_600", "diag_100")
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3.0e-310, 1.0e-40, 0.5, -0.5])


def _csr(name, dtype=np.float64, specials=False, transpose=False):
    rows, cols, I, J, V, _ = CASES[name]
    V = np.array(V, np.float64)
    if specials:
        rng = np.random.default_rng(rows * 3 + cols)
        sp = rng.random(len(V)) < 0.2
        V[sp] = rng.choice(SPECIAL, int(sp.sum()))
    rp, ci, v = sr.coo_to_csr(rows, cols, I, J, V.astype(dtype))
    return rows, cols, rp, ci, v


def _vec(n, seed, dtype, specials=True):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n)
    if specials:
        sp = rng.random(n) < 0.25
        x[sp] = rng.choice(SPECIAL, int(sp.sum()))
    return x.astype(dtype)


def _same(got, want, zero_sign=True):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    ok = (got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want))
    if not zero_sign:
        ok |= (got == 0) & (want == 0)
    return bool(np.all(ok))


def _fma64(a, x, acc):
    """fma in fp64 by exact rational arithmetic (one rounding: float(Fraction) rounds to nearest)"""
    a, x, acc = float(a), float(x), float(acc)
    if not (np.isfinite(a) and np.isfinite(x) and np.isfinite(acc)):
        return float(np.float64(a) * np.float64(x) + np.float64(acc))
    r = Fraction(a) * Fraction(x) + Fraction(acc)
    if r == 0:
        prod_neg = bool(np.signbit(a) ^ np.signbit(x))
        exact_zero_prod = a == 0 or x == 0
        return -0.0 if exact_zero_prod and acc == 0 and prod_neg and np.signbit(acc) else 0.0
    return float(r)


@pytest.mark.parametrize("accumulate", (False, True))
@pytest.mark.parametrize("transpose", (False, True))
@pytest.mark.parametrize("name", ("tiny_9x9", "rand_50", "rect_70x40_AAt", "ragged_37", "empty_rows", "cancel_and_zero", "col_vector_AAt"))
def test_plus_times_is_the_exact_fma_chain(oracle, name, transpose, accumulate):
    rows, cols, rp, ci, v = _csr(name, specials=True)
    nx, ny = (rows, cols) if transpose else (cols, rows)
    x = _vec(nx, 1, np.float64)
    y0 = _vec(ny, 2, np.float64) if accumulate else None
    if accumulate:
        y0[::3] = -0.0
    got = mr.mxv(rows, cols, rp, ci, v, x, "plus_times", np.float64, y0=y0, oracle=oracle, transpose=transpose)
    trp, tci, tv = mr.transpose_csr(rows, cols, rp, ci, v) if transpose else (rp, ci, v)
    want = np.zeros(ny)
    for i in range(ny):
        acc = y0[i] if accumulate else 0.0
        for e in range(trp[i], trp[i + 1]):
            acc = _fma64(tv[e], x[tci[e]], acc)
        want[i] = acc
    assert _same(got, want), name


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
@pytest.mark.parametrize("name", SMALL)
def test_order_independent_semirings_against_semiringref(oracle, name, dtype):
    """A (+).(x) x equals the product A * X of semiringref (X: the cols x 1 matrix storing every x_j), with start values at empty rows"""
    rows, cols, rp, ci, v = _csr(name, dtype, specials=True)
    x = _vec(cols, 5, dtype)
    X = (np.arange(cols + 1, dtype=np.int64), np.zeros(cols, np.int64), x)
    for s in mr.SEMIRINGS:
        got = mr.mxv(rows, cols, rp, ci, v, x, s, dtype, oracle=oracle)
        crp, _, cv = sr.spgemm((rp, ci, v), X, 1, s, dtype)
        want = np.full(rows, mr.MXV_START[s], dtype)
        want[np.diff(crp) > 0] = cv
        if s == "plus_times":   # semiringref sums in numpy: compare with the oracle's chain instead
            o = oracle.csr_spgemm(oracle.Csr(rows, cols, np.repeat(np.arange(rows), np.diff(rp)), ci, v.astype(np.float64)),
                                  oracle.Csr(cols, 1, np.arange(cols), np.zeros(cols, np.int64), x.astype(np.float64)),
                                  f32=dtype == np.float32).arrays()
            want = np.zeros(rows, dtype)
            want[np.diff(o[0]) > 0] = np.asarray(o[2]).astype(dtype)
        assert _same(got, want, zero_sign=s not in ("min_plus", "max_plus", "max_times")), f"{name} {s}"


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
@pytest.mark.parametrize("dim", ("rows", "cols"))
@pytest.mark.parametrize("name", SMALL)
def test_reduce_equivalences(oracle, name, dim, dtype):
    """reduce(plus) == mxv(plus_times, x = 1) bit for bit (the oracle's chain); min / max == mxv(min_plus / max_plus, x = 0) up to
    the sign of a zero; lor == mxv(lor_land, x = 1); and every fold equals numpy's own reduction where the order does not matter"""
    rows, cols, rp, ci, v = _csr(name, dtype, specials=True)
    tr = dim == "cols"
    n = rows if tr else cols
    one, zero = np.ones(n, dtype), np.zeros(n, dtype)
    kw = dict(oracle=oracle, transpose=tr)
    assert _same(mr.reduce(rows, cols, rp, ci, v, "plus", dtype, dim=dim), mr.mxv(rows, cols, rp, ci, v, one, "plus_times", dtype, **kw))
    assert _same(mr.reduce(rows, cols, rp, ci, v, "min", dtype, dim=dim), mr.mxv(rows, cols, rp, ci, v, zero, "min_plus", dtype, **kw), False)
    assert _same(mr.reduce(rows, cols, rp, ci, v, "max", dtype, dim=dim), mr.mxv(rows, cols, rp, ci, v, zero, "max_plus", dtype, **kw), False)
    assert _same(mr.reduce(rows, cols, rp, ci, v, "lor", dtype, dim=dim), mr.mxv(rows, cols, rp, ci, v, one, "lor_land", dtype, **kw))
    trp, _, tv = mr.transpose_csr(rows, cols, rp, ci, v) if tr else (rp, ci, v)
    ny = len(trp) - 1
    cnt = np.diff(trp)
    tv = np.asarray(tv, dtype)
    seg = np.minimum(trp[:-1], max(len(tv) - 1, 0))
    nz = cnt > 0
    for op, uf, ident in (("min", np.fmin, np.inf), ("max", np.fmax, -np.inf)):
        want = np.full(ny, ident, dtype)
        if len(tv):
            want[nz] = uf(dtype(ident), uf.reduceat(tv, seg))[nz]   # (a row of NaN only keeps the identity)
        assert _same(mr.reduce(rows, cols, rp, ci, v, op, dtype, dim=dim), want, False), op
    want_lor = np.zeros(ny, dtype)
    want_land = np.ones(ny, dtype)
    if len(tv):
        want_lor[nz] = np.logical_or.reduceat(tv != 0, seg)[nz]
        want_land[nz] = np.logical_and.reduceat(tv != 0, seg)[nz]
    assert _same(mr.reduce(rows, cols, rp, ci, v, "lor", dtype, dim=dim), want_lor)
    assert _same(mr.reduce(rows, cols, rp, ci, v, "land", dtype, dim=dim), want_land)
    assert _same(mr.mxv(rows, cols, rp, ci, v, one, "plus_pair", dtype, transpose=tr), cnt.astype(dtype))


def test_accumulate_folds_from_the_old_value_and_keeps_empty_rows(oracle):
    rows, cols, rp, ci, v = _csr("empty_rows")
    y0 = _vec(rows, 9, np.float64, specials=False)
    y0[:5] = [0.0, 2.0, -0.0, np.nan, 7.0]
    empty = np.diff(rp) == 0
    for s in mr.SEMIRINGS:
        got = mr.mxv(rows, cols, rp, ci, v, np.ones(cols), s, np.float64, y0=y0, oracle=oracle)
        assert _same(got[empty], y0[empty]), s
    times = mr.reduce(rows, cols, rp, ci, v, "times", np.float64, y0=y0)
    for i in np.flatnonzero(~empty)[:20]:
        acc = y0[i]
        for e in range(rp[i], rp[i + 1]):
            acc = np.float64(acc) * np.float64(v[e])
        assert _same(times[i:i + 1], np.array([acc])), i
    lor = mr.reduce(rows, cols, rp, ci, v, "lor", np.float64, y0=y0)
    assert set(np.unique(lor[~empty])) <= {0.0, 1.0} and _same(lor[empty], y0[empty])
