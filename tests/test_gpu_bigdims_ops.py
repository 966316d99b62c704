"""GPU: the operations added since test_gpu_bigdims.py part 2 was written, on the same hypersparse operand -- more than 262 144 tile
rows, tile columns and tiles, entries on both sides of tile line 262 143 | 262 144 -- where their line-walk and level-wide launches,
the pair scan's and the scan's three-launch forms, sort keys of 40 and 46 bits and kron's and concat's index arithmetic at millions of
lines run for the first time: select_topk, kron, build, concat / split, the arg folds, trsv, ilu0 / lu_solve, colour / colour_order /
reorder_by_colour, mis / aggregate / prolongator.

The entry-wise references (topkref, kronref, buildref, concatref) run plain; the others run on the lines that carry an entry and
are lifted back by the rules of tests/compactref.py, each held equal to the plain reference by tests/test_compact_cpu.py.  The
solves need a diagonal on every row: matgen.hypersparse_diag.  Every comparison is the rule of the operation's own test file, over
every entry; every test opens with the sizes it is there for and, where a regime has a kernel of its own, asserts that it ran.
"""
import numpy as np
import pytest
import torch

import aggref as ag
import argref as ar
import buildref
import colourref as cr
import compactref
import concatref
import ilu0ref
import kronref
import mxvref as mr
import topkref
import trsvref as tr
from hyperops import (DTYPES, IDS, SCAN_CHAINED_MAX, _assert_same_tiling, _bounded, _canonical, _dev, _host, _hyper, _Profiled, _same_vec,
                      bits_for, derive_passes, sort_passes)
from matgen import HYPER_N

pytestmark = pytest.mark.gpu

torch.cuda.is_available()   # (torch's runtime first, as in the other GPU files)


@pytest.fixture(scope="module")
def tctx(pkg):
    """a context on a torch stream made current for the module (as in test_gpu_mxv.py): torch's work and the library's calls are
    ordered with no extra sync"""
    prev = torch.cuda.current_stream()
    s = torch.cuda.Stream()
    torch.cuda.set_stream(s)
    c = pkg.Context(0, stream=s.cuda_stream)
    yield c
    c.close()
    torch.cuda.set_stream(prev)


def _operand_is_past(A):
    assert min(A.tile_rows, A.tile_cols, A.ntiles) > SCAN_CHAINED_MAX, "the operand is not past 262 144 tile rows, tile columns and tiles"


def _coo_tiling(pkg, ctx, rows, cols, I, J, V, dtype):
    return _bounded(pkg.Tiled.from_coo(ctx, rows, cols, I, J, np.asarray(V, dtype), dtype=dtype))


# ---- select_topk ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_hyper_select_topk(pkg, tctx, dtype):
    """rows and columns, largest and abs_largest, k = 1 and k = 3: the line walk is launched over 262 146 lines of 64 lanes"""
    H = _hyper(pkg, tctx, dtype)
    _operand_is_past(H.A)
    n = H.n
    for dim in topkref.DIMS:
        for order in ("largest", "abs_largest"):
            for k in (1, 3):
                wI, wJ, wV = topkref.select_topk(*H.coo, order, dim, k, dtype)
                assert 0 < len(wI) < len(H.I), (dim, order, k)
                R = H.A.select_topk(k, order, dim)
                # (k = 1 over the columns keeps 190 101 tiles; k = 3 keeps more than 262 144 either way, and past=True asserts it)
                _assert_same_tiling(R, _coo_tiling(pkg, tctx, n, n, wI, wJ, wV, dtype), f"select_topk {dim} {order} k={k}", past=k == 3)


# ---- kron ----------------------------------------------------------------------------------------------------------------------------
BLOCK = (3, 2, np.array([0, 0, 1, 2], np.int32), np.array([0, 1, 1, 0], np.int32), np.array([2.0, -0.5, 3.0, 0.25]))


def _kron_sorts(R):
    """the candidate tiles by (tile row, tile column), then derive_tiled's sort"""
    return sort_passes(bits_for(R.tile_rows) + bits_for(R.tile_cols)) + derive_passes(R)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("side", ["huge_left", "huge_right"])
def test_hyper_kron_and_refresh(pkg, tctx, side, dtype):
    """hypersparse (x) a 3 x 2 block of 4 entries and the block (x) hypersparse: 12 582 975 x 8 388 650, 786 436 tile rows; with the huge
    operand on the right every index of the result is divided by 4 194 325.  40-bit tile keys: five sort passes"""
    H = _hyper(pkg, tctx, dtype)
    _operand_is_past(H.A)
    n = H.n
    br, bc, bI, bJ, bV = BLOCK
    bV = bV.astype(dtype)
    B = pkg.Tiled.from_coo(tctx, br, bc, bI, bJ, bV, dtype=dtype)
    small, huge = (br, bc, bI, bJ, bV), (n, n, *H.coo)
    left, right, L, Rt = (huge, small, H.A, B) if side == "huge_left" else (small, huge, B, H.A)
    for op in (("times", "plus") if dtype == np.float64 else ("times",)):
        with _Profiled(tctx) as prof:
            K = _bounded(pkg.Tiled.kron(L, Rt, op))
        assert (K.rows, K.cols, K.tile_rows) == (3 * n, 2 * n, 786_436) and bits_for(K.tile_rows) + bits_for(K.tile_cols) == 40
        assert "scan2_reduce_kernel" in prof.names, f"kron {side} {op}: the pair scan stayed in its chained launch"
        assert prof.calls("rs_scatter_kernel") == _kron_sorts(K) == 8, (prof.calls("rs_scatter_kernel"), _kron_sorts(K))
        rows, cols, wI, wJ, wV = kronref.kron(*left, *right, op, dtype)
        _assert_same_tiling(K, _coo_tiling(pkg, tctx, rows, cols, wI, wJ, wV, dtype), f"kron {side} {op}")
    # the refresh, after set_values on both operands, against the product of the new values
    rng = np.random.default_rng(83)
    A2 = pkg.Tiled.from_coo(tctx, n, n, H.I, H.J, H.V, dtype=dtype)
    B2 = pkg.Tiled.from_coo(tctx, br, bc, bI, bJ, bV, dtype=dtype)
    L, Rt = (A2, B2) if side == "huge_left" else (B2, A2)
    K = pkg.Tiled.kron(L, Rt, "times")
    W, bW = rng.uniform(-2.0, 2.0, len(H.V)).astype(dtype), rng.uniform(-2.0, 2.0, 4).astype(dtype)
    a2, b2 = (n, n, *_canonical(H.I, H.J, W, n)), (br, bc, *_canonical(bI, bJ, bW, bc))
    A2.set_values(a2[4], "row")
    B2.set_values(b2[4], "row")
    K.set_values_from_kron(L, Rt)
    left, right = (a2, b2) if side == "huge_left" else (b2, a2)
    rows, cols, wI, wJ, wV = kronref.kron(*left, *right, "times", dtype)
    _assert_same_tiling(K, _coo_tiling(pkg, tctx, rows, cols, wI, wJ, wV, dtype), f"set_values_from_kron {side}")


# ---- build ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_hyper_build_and_refresh(pkg, tctx, dtype):
    """the hypersparse triplets with runs of 1 to 5 duplicates, shuffled: 46-bit sort keys (8 in-tile bits + 19 + 19), six passes, so the
    sorted keys end in the first buffer again -- build's own tests stop at 34 bits, five passes, where they end in the second"""
    H = _hyper(pkg, tctx, dtype)
    _operand_is_past(H.A)
    n = H.n
    rng = np.random.default_rng(89)
    tI, tJ, tV = buildref.with_duplicates(H.I, H.J, H.V, rng, rng.integers(1, 6, len(H.I)))
    assert len(tI) > 2 * len(H.I) and tV.dtype == dtype
    for op in (("plus", "first", "second") if dtype == np.float64 else ("plus",)):
        with _Profiled(tctx) as prof:
            T = _bounded(pkg.Tiled.build(tctx, n, n, tI, tJ, tV, dup=op, dtype=dtype))
        key_bits = 8 + bits_for(T.tile_rows) + bits_for(T.tile_cols)
        assert key_bits == 46
        assert "scan2_reduce_kernel" in prof.names, f"build {op}: the pair scan stayed in its chained launch"
        assert prof.calls("rs_scatter_kernel") == sort_passes(key_bits) + derive_passes(T) == 9, prof.calls("rs_scatter_kernel")
        oI, oJ, oV = buildref.fold(n, n, tI, tJ, tV, op)
        assert len(oI) == len(H.I)
        _assert_same_tiling(T, _coo_tiling(pkg, tctx, n, n, oI, oJ, oV, dtype), f"build {op}")
    T = pkg.Tiled.build(tctx, n, n, tI, tJ, tV, dup="plus", dtype=dtype, keep_map=True)
    W = rng.uniform(-2.0, 2.0, len(tV)).astype(dtype)
    dW = _dev(W)                                             # (kept alive until the context's stream has read it)
    T.set_values_from_build(dW)
    tctx.synchronize()
    oI, oJ, oV = buildref.fold(n, n, tI, tJ, W, "plus")
    _assert_same_tiling(T, _coo_tiling(pkg, tctx, n, n, oI, oJ, oV, dtype), "set_values_from_build")


# ---- concat / split ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_hyper_concat_refresh_and_split(pkg, tctx, dtype):
    """[[H, None], [H^T, H]]: 8 388 650 square, the offsets 4 194 325 -- no multiple of 16, so every tile of the lower and the right
    blocks is cut and reassembled -- 40-bit tile keys"""
    H = _hyper(pkg, tctx, dtype)
    _operand_is_past(H.A)
    n = H.n
    assert n % 16 != 0
    At = pkg.Tiled.from_coo(tctx, n, n, H.I, H.J, H.V, True, dtype=dtype)
    a, at = H.coo, _canonical(H.J, H.I, H.V, n)
    with _Profiled(tctx) as prof:
        R = _bounded(pkg.Tiled.concat([[H.A, None], [At, H.A]]))
    assert (R.rows, R.cols) == (2 * n, 2 * n) and bits_for(R.tile_rows) + bits_for(R.tile_cols) == 40
    assert "scan2_reduce_kernel" in prof.names, "concat: the pair scan stayed in its chained launch"
    assert prof.calls("rs_scatter_kernel") == _kron_sorts(R) == 8, prof.calls("rs_scatter_kernel")
    rows, cols, wI, wJ, wV = concatref.concat([[a, None], [at, a]], [n, n], [n, n], dtype)
    _assert_same_tiling(R, _coo_tiling(pkg, tctx, rows, cols, wI, wJ, wV, dtype), "concat")
    pieces = R.split([n, n], [n, n])
    none = np.zeros(0, np.int32)
    empty = pkg.Tiled.from_coo(tctx, n, n, none, none, np.zeros(0, dtype), dtype=dtype)
    for (i, j), want in (((0, 0), H.A), ((0, 1), empty), ((1, 0), At), ((1, 1), H.A)):
        _assert_same_tiling(pieces[i][j], want, f"split piece ({i}, {j})", past=want is not empty)
    if dtype != np.float64:
        return
    rng = np.random.default_rng(97)
    A2 = pkg.Tiled.from_coo(tctx, n, n, H.I, H.J, H.V, dtype=dtype)
    At2 = pkg.Tiled.from_coo(tctx, n, n, H.I, H.J, H.V, True, dtype=dtype)
    grid = [[A2, None], [At2, A2]]
    R2 = pkg.Tiled.concat(grid)
    W, Wt = rng.uniform(-2.0, 2.0, len(H.V)).astype(dtype), rng.uniform(-2.0, 2.0, len(H.V)).astype(dtype)
    a2, at2 = _canonical(H.I, H.J, W, n), _canonical(H.J, H.I, Wt, n)
    A2.set_values(a2[2], "row")
    At2.set_values(at2[2], "row")
    R2.set_values_from_concat(grid)
    rows, cols, wI, wJ, wV = concatref.concat([[a2, None], [at2, a2]], [n, n], [n, n], dtype)
    _assert_same_tiling(R2, _coo_tiling(pkg, tctx, rows, cols, wI, wJ, wV, dtype), "set_values_from_concat")


# ---- the arg folds -------------------------------------------------------------------------------------------------------------------
def _present_1000(H, rng):
    present = np.zeros(H.n, np.uint8)
    present[np.concatenate([rng.choice(H.map.used, 900, replace=False), H.S[:60], rng.integers(0, H.n, 40)])] = 1
    present[np.flatnonzero(present)[1000:]] = 0
    assert present.sum() == 1000
    return present


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("tr_", [False, True], ids=("Ax", "ATx"))
@pytest.mark.parametrize("kind", ["min_plus", "max_times", "min_index"])
def test_hyper_mxv_arg(pkg, tctx, kind, tr_, dtype):
    """a 1 000-entry x_present, accumulate off and on, against argref on the used lines; an absent line takes the start value and
    -1, or with accumulate keeps what it held"""
    H = _hyper(pkg, tctx, dtype)
    _operand_is_past(H.A)
    n, m = H.n, H.map
    rng = np.random.default_rng(101)
    x, y0 = rng.standard_normal(n).astype(dtype), rng.standard_normal(n).astype(dtype)
    present = _present_1000(H, rng)
    i0 = np.where(rng.random(n) < 0.5, -1, m.used[rng.integers(0, m.cdim, n)]).astype(np.int32)
    i0c = np.where(m.gather(i0) >= 0, np.searchsorted(m.used, np.maximum(m.gather(i0), 0)), -1).astype(np.int32)
    values = kind in ar.VALUE_KINDS
    dx, dp = _dev(x), _dev(present)
    for acc in (False, True):
        old = dict(y_old=m.gather(y0), idx_old=i0c, accumulate=True) if acc else {}
        yc, ic, pc = ar.mxv_arg(m.cdim, m.cdim, *H.ccsr, m.gather(x), kind, dtype, present=m.gather(present), transpose=tr_, **old)
        out = _dev(y0) if acc and values else None
        oidx = _dev(i0) if acc else None
        opres = torch.zeros(n, dtype=torch.uint8, device="cuda")
        gy, gi = H.A.mxv_arg(dx, kind, tr_, x_present=dp, out=out, out_index=oidx, out_present=opres, accumulate=acc)
        label = f"mxv_arg {kind} transpose={tr_} accumulate={acc}"
        if values:
            assert _same_vec(_host(gy), m.scatter(yc, y0 if acc else ar.START[kind]), kind), f"{label}: values"
        else:
            assert gy is None
        assert np.array_equal(_host(gi), compactref.lift_index(m, ic, i0 if acc else -1)), f"{label}: index"
        want_p = m.scatter(pc, 0)
        assert np.array_equal(_host(opres), want_p) and 0 < want_p.sum() < 16 * 1000, f"{label}: presence"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("dim", ["rows", "cols"])
def test_hyper_reduce_arg(pkg, tctx, dim, dtype):
    H = _hyper(pkg, tctx, dtype)
    _operand_is_past(H.A)
    m = H.map
    for op in ("min", "max"):
        yc, ic = ar.reduce_arg(m.cdim, m.cdim, *H.ccsr, op, dtype, dim=dim)
        gy, gi = H.A.reduce_arg(op, dim)
        assert _same_vec(_host(gy), m.scatter(yc, mr.IDENTITY[op]), op), f"reduce_arg {op} {dim}: values"
        want = compactref.lift_index(m, ic)
        assert np.array_equal(_host(gi), want) and (want < 0).sum() == H.n - len(np.unique(H.I if dim == "rows" else H.J))


@pytest.mark.parametrize("source", [0, HYPER_N - 1])
def test_hyper_bfs_parents(pkg, tctx, source):
    """levels equal bfs's; every parent is a candidate parent -- one level up, with a stored edge to the vertex -- and the least of
    them, which is argref's"""
    H = _hyper(pkg, tctx, np.float64)
    _operand_is_past(H.A)
    n, m = H.n, H.map
    keys = np.sort(H.I.astype(np.int64) * n + H.J)
    for tr_ in (False, True):
        lvc, pac, depth, reached = ar.bfs_parents(m.cdim, H.ccsr[0], H.ccsr[1], int(np.searchsorted(m.used, source)), tr_)
        lv, pa, d, r = H.A.bfs_parents(source, tr_)
        blv, bd, br = H.A.bfs(source, tr_)
        lv, pa = _host(lv), _host(pa)
        assert np.array_equal(lv, _host(blv)) and (d, r) == (bd, br), "levels differ from bfs"
        assert (d, r) == (depth, reached) and reached > 400 and depth >= 2, (source, tr_, d, r)
        assert np.array_equal(lv, m.scatter(lvc, -1))
        v = np.flatnonzero(lv > 0)
        p = pa[v].astype(np.int64)
        assert np.all(p >= 0) and np.array_equal(lv[p], lv[v] - 1), "a parent is not one level up"
        edge = v * n + p if tr_ else p * n + v                              # (i, j) stored: i -> j; transposed: j -> i
        assert np.all(keys[np.minimum(np.searchsorted(keys, edge), len(keys) - 1)] == edge), "a parent without an edge to its vertex"
        assert pa[source] == source and np.all(pa[lv < 0] == -1)
        cand = ar.candidate_parents(m.cdim, H.ccsr[0], H.ccsr[1], lvc, tr_)
        assert (cand[lvc > 0] > 1).any(), "no vertex has two candidate parents: the least-parent rule is not exercised"
        assert np.array_equal(pa, compactref.lift_index(m, pac)), "parents differ from the model's"


# ---- trsv ----------------------------------------------------------------------------------------------------------------------------
def _system(H):
    """(the IndexMap of the rows with an off-diagonal entry, their compacted CSR, its mask in the whole (row, col) order, the diagonal)"""
    def make():
        om = H.offmap()
        ccsr, kept = compactref.compact_system(om, H.I, H.J, H.V)
        d = np.zeros(H.n, H.dtype)
        on = H.I == H.J
        d[H.I[on]] = H.V[on]
        assert np.all(d != 0)
        return om, ccsr, kept, d
    return H.cached("system", make)


def _solve_ref(H, om, ccsr, b, uplo, unit, d):
    x = tr.trsv(om.cdim, *ccsr, om.gather(b), uplo, unit, H.dtype, index=om.used)
    return compactref.lift_solution(om, x, b, None if unit else d)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_hyper_trsv(pkg, tctx, dtype):
    """both triangles, with and without unit_diag, merged and one launch per level; the first level is some 160 000 tile rows wide,
    where the tests of trsv itself stop at a few hundred.  trsvref runs on the rows with an off-diagonal entry under index=, so the
    upper walk keeps the original tile edges; the other rows are b_i / a_ii"""
    H = _hyper(pkg, tctx, dtype, diag=True)
    _operand_is_past(H.A)
    n = H.n
    om, ccsr, kept, d = _system(H)
    assert SCAN_CHAINED_MAX < om.cdim < n and H.A.nnz > 4_400_000
    b = np.random.default_rng(103).standard_normal(n).astype(dtype)
    db = _dev(b)
    extra = H.A.tile_rows - len(np.unique(om.used // 16))               # tile rows whose rows all stand alone: level 1
    wants = {}
    for uplo in tr.UPLO:
        lv = np.concatenate([tr.levels(om.cdim, ccsr[0], ccsr[1], uplo, index=om.used), np.ones(extra, np.int64)])
        ws = tr.widths(lv)
        assert ws[0] == max(ws) > 100_000 and len(ws) > 8, ws[:4]
        for unit in (False, True):
            want = wants[uplo, unit] = _solve_ref(H, om, ccsr, b, uplo, unit, d)
            try:
                for split in (False, True):
                    tctx.trsv_split(split)
                    got = _host(H.A.trsv(db, uplo, unit))
                    assert _same_vec(got, want), f"trsv {uplo} unit={unit} split={split}: {int(np.sum(got != want))} of {n} differ"
                    info = H.A.trsv_info(uplo)
                    assert info["levels"] == len(ws) and info["max_width"] == ws[0], (uplo, info)
                    assert info["missing_diag"] == 0 and info["first_missing_row"] == 0
                    if split:
                        assert info["merge_width"] == 0 and info["launches"] == len(ws), info
                    else:
                        assert info["merge_width"] >= 4 and info["launches"] == tr.launches(lv, info["merge_width"]), info
            finally:
                tctx.trsv_split(False)
    # new values on the same tiling: the schedule stays, the solve reads them
    A2 = pkg.Tiled.from_coo(tctx, n, n, H.I, H.J, H.V, dtype=dtype)
    x0 = _host(A2.trsv(db, "upper"))
    assert _same_vec(x0, wants["upper", False])
    W = (H.V * np.random.default_rng(107).uniform(0.5, 2.0, len(H.V))).astype(dtype)
    Ws = _canonical(H.I, H.J, W, n)[2]
    dW = _dev(Ws)
    A2.set_values_device(dW, "row")
    d2 = np.zeros(n, dtype)
    d2[H.I[H.I == H.J]] = W[H.I == H.J]
    x = tr.trsv(om.cdim, ccsr[0], ccsr[1], Ws[kept], om.gather(b), "upper", False, dtype, index=om.used)
    got = _host(A2.trsv(db, "upper"))
    assert _same_vec(got, compactref.lift_solution(om, x, b, d2)), "trsv after set_values_device"
    assert not _same_vec(got, x0)


# ---- ilu0 / lu_solve -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_hyper_ilu0_and_lu_solve(pkg, tctx, dtype):
    H = _hyper(pkg, tctx, dtype, diag=True)
    _operand_is_past(H.A)
    n = H.n
    om, ccsr, kept, d = _system(H)
    cI, cJ, cV = H.coo
    fc, longest = ilu0ref.ilu0(om.cdim, *ccsr, dtype)
    assert longest >= 2, "no entry of the factor takes more than one fma"
    F = H.A.ilu0()
    _assert_same_tiling(F, _coo_tiling(pkg, tctx, n, n, cI, cJ, compactref.lift_factor(kept, fc, cV), dtype), "ilu0")
    extra = H.A.tile_rows - len(np.unique(om.used // 16))
    lv = np.concatenate([tr.levels(om.cdim, ccsr[0], ccsr[1], "lower", index=om.used), np.ones(extra, np.int64)])
    ws = tr.widths(lv)
    info = F.ilu0_info()
    assert info["levels"] == len(ws) and info["max_width"] == ws[0] > 100_000, info
    assert info["zero_pivots"] == 0 and info["first_zero_pivot_row"] == 0
    assert info["merge_width"] >= 4 and info["launches"] == tr.launches(lv, info["merge_width"]), info
    # lu_solve: lower-unit, then upper, on the factor
    b = np.random.default_rng(109).standard_normal(n).astype(dtype)
    w = tr.trsv(om.cdim, ccsr[0], ccsr[1], fc, om.gather(b), "lower", True, dtype, index=om.used)
    z = tr.trsv(om.cdim, ccsr[0], ccsr[1], fc, w, "upper", False, dtype, index=om.used)
    got = _host(F.lu_solve(_dev(b)))
    assert _same_vec(got, compactref.lift_solution(om, z, b, d)), f"lu_solve: {int(np.sum(got != compactref.lift_solution(om, z, b, d)))} differ"
    # the refresh: new values by the operand's recipe (still diagonally dominant), against the reference's factor of them
    rng = np.random.default_rng(113)
    off = H.I != H.J
    W = np.array(H.V)
    W[off] = rng.uniform(-1.0, 1.0, int(off.sum())).astype(dtype)
    W[~off] = (4.0 + np.bincount(H.I[off], weights=np.abs(W[off]).astype(np.float64), minlength=n))[H.I[~off]].astype(dtype)
    Ws = _canonical(H.I, H.J, W, n)[2]
    A2 = pkg.Tiled.from_coo(tctx, n, n, H.I, H.J, H.V, dtype=dtype)
    F2 = A2.ilu0()
    A2.set_values(Ws, "row")
    F2.set_values_from_ilu0(A2)
    f2, _ = ilu0ref.ilu0(om.cdim, ccsr[0], ccsr[1], Ws[kept], dtype)
    _assert_same_tiling(F2, _coo_tiling(pkg, tctx, n, n, cI, cJ, compactref.lift_factor(kept, f2, Ws), dtype), "set_values_from_ilu0")
    assert F2.ilu0_info()["zero_pivots"] == 0


# ---- colour / colour_order / reorder_by_colour ------------------------------------------------------------------------------------------
def _graph(H):
    """(the IndexMap of the vertices with a neighbour, the compacted off-diagonal pattern, a priority per vertex)"""
    def make():
        om = H.offmap()
        cI, cJ = compactref.compact_pattern(om, H.I, H.J)
        prio = np.random.default_rng(127).integers(0, 2 ** 32, H.n).astype(np.uint32)
        return om, cI, cJ, prio
    return H.cached("graph", make)


def test_hyper_colour_order_and_reorder(pkg, tctx):
    """colours, ncolours and rounds against colourref's greedy colouring of the vertices with a neighbour (the others: colour 0), under
    symmetric=False on the pattern as stored and under symmetric=True where the promise holds, on the pattern united with its
    transpose; colour_order sorts 4 194 325 keys in 1 025 blocks, whose 262 400-word histogram scan takes three launches"""
    H = _hyper(pkg, tctx, np.float64)
    _operand_is_past(H.A)
    n = H.n
    om, cI, cJ, prio = _graph(H)
    assert SCAN_CHAINED_MAX < om.cdim < n
    sI, sJ = cr.symmetrised(H.I, H.J)
    S = pkg.Tiled.from_coo(tctx, n, n, sI, sJ, np.ones(len(sI)))
    _operand_is_past(S)
    cc, nc, rounds = cr.colouring(om.cdim, cI, cJ, priority=prio[om.used])
    want = compactref.lift_colours(om, cc)
    assert nc > 2 and rounds > 2
    dprio = _dev(prio.view(np.int32))
    for symmetric, A in ((False, H.A), (True, S)):
        c, gnc, grounds = A.colour(priority=dprio, symmetric=symmetric)
        assert (gnc, grounds) == (nc, rounds), (symmetric, gnc, grounds, nc, rounds)
        assert np.array_equal(_host(c), want), f"colour symmetric={symmetric}"
    seed = 12345
    cc, snc, srounds = cr.colouring(om.cdim, cI, cJ, priority=cr.hash_priority_at(om.used, seed))
    c, gnc, grounds = H.A.colour(seed=seed)
    assert (gnc, grounds) == (snc, srounds) and np.array_equal(_host(c), compactref.lift_colours(om, cc)), "colour by the default hash"
    # colour_order of the device's colours
    assert -(-n // 4096) == 1025 and 256 * 1025 > SCAN_CHAINED_MAX
    with _Profiled(tctx) as prof:
        perm, offsets = pkg.colour_order(tctx, c, gnc)
    assert "scan_reduce_kernel" in prof.names, "colour_order: the histogram scan stayed in its chained launch"
    assert prof.calls("rs_scatter_kernel") == sort_passes(bits_for(gnc)) == 1
    wperm, woffsets = cr.colour_order(_host(c), gnc)
    assert np.array_equal(_host(perm), wperm) and np.array_equal(_host(offsets), woffsets)
    # reorder_by_colour: the same order, and R = extract(p, p) = the entries renamed
    R, rperm, roffsets = H.A.reorder_by_colour(seed=seed)
    assert np.array_equal(_host(rperm), wperm) and np.array_equal(_host(roffsets), woffsets)
    _assert_same_tiling(R, H.A.extract(perm, perm), "reorder_by_colour against extract(p, p)", past=False)
    assert R.nnz == H.A.nnz and R.tile_rows > SCAN_CHAINED_MAX
    inv = np.empty(n, np.int32)
    inv[wperm] = np.arange(n, dtype=np.int32)
    _assert_same_tiling(R, pkg.Tiled.from_coo(tctx, n, n, inv[H.I], inv[H.J], H.V), "reorder_by_colour against the renamed entries", past=False)


# ---- mis / aggregate / prolongator -----------------------------------------------------------------------------------------------------
def test_hyper_mis_aggregate_and_prolongator(pkg, tctx):
    """the sets at distance 1 and 2 and the aggregation against aggref on the vertices with a neighbour: a vertex without one is in
    every set and the root of its own aggregate, so about 3.9 million roots are ranked by a scan over n in its three-launch form"""
    H = _hyper(pkg, tctx, np.float64)
    _operand_is_past(H.A)
    n = H.n
    om, cI, cJ, prio = _graph(H)
    dprio = _dev(prio.view(np.int32))
    pc = prio[om.used]
    for distance in (1, 2):
        sc, count_c, rounds = ag.mis(om.cdim, cI, cJ, distance, priority=pc)
        want, count = compactref.lift_mis(om, sc, count_c)
        with _Profiled(tctx) as prof:
            s, gcount, grounds = H.A.mis(distance, priority=dprio)
        assert "scan_reduce_kernel" in prof.names, f"mis distance={distance}: no scan took the three-launch form"
        assert (gcount, grounds) == (count, rounds) and rounds > 2, (distance, gcount, grounds, count, rounds)
        assert np.array_equal(_host(s), want), f"mis distance={distance}"
    ac, rc, ncc, rounds = ag.aggregate(om.cdim, cI, cJ, priority=pc)
    wagg, wroots, wnc = compactref.lift_aggregate(om, ac, rc, ncc)
    with _Profiled(tctx) as prof:
        agg, roots, gnc, grounds = H.A.aggregate(priority=dprio)
    assert "scan_reduce_kernel" in prof.names, "aggregate: the rank scan stayed in its chained launch"
    assert (gnc, grounds) == (wnc, rounds) and wnc > SCAN_CHAINED_MAX
    assert np.array_equal(_host(agg), wagg) and np.array_equal(_host(roots), wroots)
    P = _bounded(pkg.prolongator(tctx, agg, gnc))
    want = pkg.Tiled.from_coo(tctx, n, wnc, np.arange(n, dtype=np.int32), wagg, np.ones(n))
    _assert_same_tiling(P, want, "prolongator", past=False)                # (3 982 741 aggregates are 248 922 tile columns)
    assert min(P.tile_rows, P.ntiles) > SCAN_CHAINED_MAX and P.nnz == n
