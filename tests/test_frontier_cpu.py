"""CPU: the numpy model of the frontier products and the breadth-first search (frontierref.py) against a per-entry Python loop and
against mxvref -- the yardstick the GPU tests of pem_tiled_mxv_frontier / pem_tiled_bfs use."""
from fractions import Fraction

import numpy as np
import pytest

import frontierref as fr
import mxvref as mr
import semiringref as sr
from matgen import cases

CASES = cases()
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3.0e-310, 1.0e-40, 0.5, -0.5])
MINMAX = ("min_plus", "max_plus", "max_times")


def _csr(name, dtype=np.float64, specials=True):
    rows, cols, I, J, V, _ = CASES[name]
    V = np.array(V, np.float64)
    if specials:
        rng = np.random.default_rng(rows * 3 + cols)
        sp = rng.random(len(V)) < 0.2
        V[sp] = rng.choice(SPECIAL, int(sp.sum()))
    rp, ci, v = sr.coo_to_csr(rows, cols, I, J, V.astype(dtype))
    return rows, cols, np.asarray(rp, np.int64), np.asarray(ci, np.int64), v


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
    """fma in fp64 by exact rational arithmetic on finite operands (one rounding)"""
    a, x, acc = float(a), float(x), float(acc)
    r = Fraction(a) * Fraction(x) + Fraction(acc)
    if r == 0:
        neg = bool(np.signbit(a) ^ np.signbit(x))
        return -0.0 if (a == 0 or x == 0) and neg and np.signbit(acc) else 0.0
    return float(r)


def _loop(rows, cols, rp, ci, v, x, s, dtype, present, mask, complement, y_old, accumulate, transpose):
    """the contract of pem_tiled_mxv_frontier read entry by entry"""
    t = dtype
    if transpose:
        rp, ci, v = mr.transpose_csr(rows, cols, rp, ci, v)
        rows, cols = cols, rows
    y, pres = np.array(y_old, dtype), np.zeros(rows, np.uint8)
    with np.errstate(all="ignore"):
        for i in range(rows):
            if mask is not None and (mask[i] != 0) == bool(complement):
                continue
            acc = t(mr.MXV_START[s])
            if accumulate:
                acc = t(y_old[i] != 0) if s == "lor_land" else t(y_old[i])
            n = 0
            for e in range(rp[i], rp[i + 1]):
                j = ci[e]
                if present is not None and not present[j]:
                    continue
                n += 1
                a = t(v[e])
                if s == "plus_pair":
                    acc = t(acc + t(1))
                    continue
                xv = t(x[j])
                if s == "plus_times":
                    acc = t(_fma64(a, xv, acc))
                elif s == "min_plus":
                    acc = np.fmin(acc, t(a + xv))
                elif s == "max_plus":
                    acc = np.fmax(acc, t(a + xv))
                elif s == "max_times":
                    acc = np.fmax(acc, t(a * xv))
                else:
                    acc = t(1) if (a != 0 and xv != 0) else acc
            if n or not accumulate:
                y[i] = acc
            pres[i] = n > 0
    return y, pres


PRESENCE = ("none", "all", "one", "half")
MASKS = ((None, False), ("half", False), ("half", True), ("off", False), ("off", True))


@pytest.mark.parametrize("accumulate", (False, True))
@pytest.mark.parametrize("transpose", (False, True))
@pytest.mark.parametrize("name", ("tiny_9x9", "one_entry", "ragged_37"))
def test_model_equals_the_per_entry_loop(oracle, name, transpose, accumulate):
    rng = np.random.default_rng(5)
    for dtype in (np.float64, np.float32):
        for s in mr.SEMIRINGS:
            if s == "plus_times" and dtype == np.float32:
                continue   # (the loop's exact fma is fp64)
            finite = s == "plus_times"   # the rational fma takes finite operands
            rows, cols, rp, ci, v = _csr(name, dtype, specials=not finite)
            nx, ny = (rows, cols) if transpose else (cols, rows)
            x = _vec(nx, 1, dtype, specials=not finite)
            y_old = _vec(ny, 2, dtype, specials=not finite)
            for pk in PRESENCE:
                present = {"none": np.zeros(nx, bool), "all": None, "one": np.arange(nx) == nx // 2, "half": rng.random(nx) < 0.5}[pk]
                for mk, comp in MASKS:
                    mask = None if mk is None else (rng.random(ny) < 0.5 if mk == "half" else np.zeros(ny, bool)).astype(np.uint8) * 3
                    got, gp = fr.mxv_frontier(rows, cols, rp, ci, v, x, s, dtype, present, mask, comp, y_old, accumulate, oracle, transpose)
                    want, wp = _loop(rows, cols, rp, ci, v, x, s, dtype, present, mask, comp, y_old, accumulate, transpose)
                    label = f"{name} {s} {np.dtype(dtype).name} present={pk} mask={mk} complement={comp}"
                    assert _same(got, want, zero_sign=s not in MINMAX), label
                    assert np.array_equal(gp, wp), label


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
@pytest.mark.parametrize("name", ("tiny_9x9", "one_entry", "ragged_37", "rect_33x65_AAt", "empty_rows", "powerlaw_600"))
def test_all_present_and_no_mask_is_mxv(oracle, name, dtype):
    rows, cols, rp, ci, v = _csr(name, dtype)
    for tr in (False, True):
        nx, ny = (rows, cols) if tr else (cols, rows)
        x, y_old = _vec(nx, 3, dtype), _vec(ny, 4, dtype)
        trp = mr.transpose_csr(rows, cols, rp, ci, v)[0] if tr else rp
        for s in mr.SEMIRINGS:
            for acc in (False, True):
                got, pres = fr.mxv_frontier(rows, cols, rp, ci, v, x, s, dtype, y_old=y_old, accumulate=acc, oracle=oracle, transpose=tr)
                want = mr.mxv(rows, cols, rp, ci, v, x, s, dtype, y0=y_old if acc else None, oracle=oracle, transpose=tr)
                assert _same(got, want), f"{name} {s} transpose={tr} accumulate={acc}"
                assert np.array_equal(pres, (np.diff(trp) > 0).astype(np.uint8))
                ones = np.ones(nx, np.uint8)
                again, _ = fr.mxv_frontier(rows, cols, rp, ci, v, x, s, dtype, ones, np.ones(ny, np.uint8), False, y_old, acc, oracle, tr)
                assert _same(again, want)


def test_absent_values_cannot_reach_the_model(oracle):
    rows, cols, rp, ci, v = _csr("ragged_37", specials=False)
    present = np.random.default_rng(1).random(cols) < 0.5
    x = _vec(cols, 7, np.float64, specials=False)
    poisoned = x.copy()
    poisoned[~present] = np.nan
    for s in mr.SEMIRINGS:
        a, _ = fr.mxv_frontier(rows, cols, rp, ci, v, x, s, np.float64, present, oracle=oracle)
        b, _ = fr.mxv_frontier(rows, cols, rp, ci, v, poisoned, s, np.float64, present, oracle=oracle)
        assert _same(a, b) and not np.isnan(a).any(), s


def test_line_flags_follow_the_tile_rule():
    rows, cols, rp, ci, v = _csr("ragged_37")
    I = np.repeat(np.arange(rows), np.diff(rp))
    for tr in (False, True):
        major, minor, nx = (ci, I, rows) if tr else (I, ci, cols)
        for present in (np.zeros(nx, bool), np.ones(nx, bool), np.arange(nx) == nx - 1, np.arange(nx) == 17):
            want = np.zeros(((cols if tr else rows) + 15) // 16, np.uint8)
            for a, b in zip(major, minor):   # a tile (a // 16, b // 16) whose segment b // 16 has a present entry flags line a // 16
                if present[16 * (b // 16):16 * (b // 16) + 16].any():
                    want[a // 16] = 1
            assert np.array_equal(fr.line_flags(rows, cols, rp, ci, present, tr), want)


def test_bfs_model_on_a_path_and_a_star():
    n = 6   # 0 -> 1 -> 2 -> 3, 0 -> 4, and 5 alone
    I, J = np.array([0, 1, 2, 0]), np.array([1, 2, 3, 4])
    rp, ci, _ = sr.coo_to_csr(n, n, I, J, np.ones(4))
    lv, depth, reached = fr.bfs(n, rp, ci, 0)
    assert lv.tolist() == [0, 1, 2, 3, 1, -1] and (depth, reached) == (3, 5)
    lv, depth, reached = fr.bfs(n, rp, ci, 3, transpose=True)
    assert lv.tolist() == [3, 2, 1, 0, -1, -1] and (depth, reached) == (3, 4)
    lv, depth, reached = fr.bfs(n, rp, ci, 5)
    assert lv.tolist() == [-1] * 5 + [0] and (depth, reached) == (0, 1)
