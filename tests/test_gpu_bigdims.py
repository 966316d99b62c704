"""GPU: the code paths that the DIMENSIONS of a matrix select, at the smallest dimensions that select them.

Part 1, the key-width ladder: A*A^T with B = A^T of 2^19 + 1, 2^21 + 1 and 2^23 + 1 tile columns, where step 1's row bins switch to
64-bit keys one after another and sort real bits above 32.  Part 2: a hypersparse square tiling with more than 262 144 tile rows,
tile columns and tiles -- the length at which the device scan leaves its single chained launch -- through every operation.  Part 3:
a conversion of more than 4 194 304 entries, where the radix sort's histogram scan leaves that launch too.

The references run on the operands with their empty 16-line blocks squeezed out and are lifted back (tests/compactref.py, proved
equal to the plain oracle by tests/test_compact_cpu.py), so they cost by the entries.  Every case asserts that it reached its
regime: the kernels that ran, or the threshold it is past.
"""
import numpy as np
import pytest
import torch

import assignref as asg
import chainref
import compactref
import ewiseref as ew
import extractref as ex
import frontierref as fr
import maskref
import mxvref as mr
import sddmmref as sd
import selectref as sel
import semiringref as sr
import spmmref as sp
from compactref import T_NAMES, Product, lift_coo, lift_csr, lift_plan_arrays
from hyperops import (DTYPES, IDS, SCAN_CHAINED_MAX, SORT_BLOCK_KEYS, _assert_same_tiling, _canonical, _dev, _host, _hyper, _Profiled, _same,
                      _same_vec)
from matgen import BIGDIM_RUNGS, HYPER_N, bigdim_case
from prune_ref import C_NAMES, expected
from s3cases import poisoned

pytestmark = pytest.mark.gpu

torch.cuda.is_available()   # (torch's runtime first, as in the other GPU files)

def _check_tiled(g, lifted, label, vals=None):
    """every tiled array of the device tiling g against a compactref.LiftedTiled (vals: the expected values in another dtype)"""
    assert (g.rows, g.cols, g.nnz, g.tile_rows, g.tile_cols, g.ntiles) == \
        (lifted.rows, lifted.cols, lifted.nnz, lifted.tile_rows, lifted.tile_cols, lifted.ntiles), label
    for arr in T_NAMES:
        got = g.array(arr)
        if arr == "vals" and vals is not None:
            assert _same(got, vals), f"{label}: tiled array vals differs"
        else:
            assert lifted.matches(arr, got), f"{label}: tiled array {arr} differs"


# ------------------------------------------------------------------------------------------------------------------------------
# part 1: the key-width ladder
# ------------------------------------------------------------------------------------------------------------------------------
_RUNG = {}


def _rung(pkg, oracle, ctx, rung):
    """(case, compacted reference, device A, device A^T, lifted COO of the serial CSR product) -- once per session"""
    if rung not in _RUNG:
        case = bigdim_case(rung)
        rows, cols, I, J, V, tr = case
        ref = Product(oracle, case)
        gA = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, False)
        gB = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, True)
        assert gB.tile_cols == BIGDIM_RUNGS[rung] + 1 > 1 << (rung - 1), "B does not reach the rung"
        assert gA.tile_rows > SCAN_CHAINED_MAX
        _RUNG[rung] = (case, ref, gA, gB, ref.csr_spgemm_coo()[0])
    return _RUNG[rung]


def _ladder_kernels(rung, segments, xl_global):
    """(names that must have run, names that must not) in one pass of step 1 at a rung: bin k sorts 64-bit keys where the rung's
    tile-column bits + its index bits (9, 11, 13) exceed 32"""
    must, never = {"s1_tiny_kernel", "s1_rowclass_kernel", "scan_reduce_kernel"}, {"s1_bins_kernel", "s1_rowclass_kernel<scan>",
                                                                                  "s1_rowsort_kernel<32768>", "s1_rowsort_big_kernel"}
    for cap, qb in ((512, 9), (2048, 11), (8192, 13)):
        wide, narrow = f"s1_rowsort_kernel<{cap},key64>", f"s1_rowsort_kernel<{cap}>"
        (must if rung + qb > 32 else never).add(wide)
        (never if rung + qb > 32 else must).add(narrow)
    seg = ("s1_rowseg_kernel<key64>", "s1_rowseg_kernel") if rung + 11 > 32 else ("s1_rowseg_kernel", "s1_rowseg_kernel<key64>")
    xl = ("s1_xl_emit_kernel", "s1_xl_rowsort_kernel") if xl_global else ("s1_xl_rowsort_kernel", "s1_xl_emit_kernel")
    if segments:
        must.add(seg[0])
        never.update({seg[1], "s1_xl_gather_kernel", *xl})
    else:
        must.update({"s1_xl_gather_kernel", xl[0]})
        never.update({xl[1], *seg})
    return must, never


def _check_plan(plan, ref, want_arrays, want_counts, coo, label, csr):
    info = plan.info()
    assert (info["ntiles_c"], info["npairs"], info["nnz_c"], info["npairs_all"]) == want_counts, label
    lifted = lift_plan_arrays(want_arrays, ref.rmap, ref.cmap, expand=False)
    for arr in C_NAMES:
        got = plan.array(arr)
        if arr == "c_tile_rowptr":     # compared at the used tile rows: no reference as long as the dimension
            assert ref.rmap.ptr_matches(got, lifted[arr]), f"{label}: plan array {arr} differs"
        else:
            assert _same(got, lifted[arr]), f"{label}: plan array {arr} differs"
    assert not poisoned(plan.array("c_vals")).any(), f"{label}: step 3 left entries unwritten"
    r, c, v = plan.export_coo()
    for got, want in zip((r, c, v), lift_coo(*ref.op.export_coo(), ref.rmap, ref.cmap)):
        assert _same(got, want), f"{label}: export_coo differs from the tiled oracle"
    assert _same(r, coo[0]) and _same(c, coo[1]), f"{label}: export_coo differs from the serial CSR product"
    assert _same(v, coo[2]), f"{label}: values must match the ascending-k fma chain bit for bit"
    if csr:                            # (a rowptr is as long as the dimension: only where that is small)
        for got, want in zip(plan.export_csr(), lift_csr(*ref.op.export_csr(), ref.rmap, ref.cmap)):
            assert _same(got, want), f"{label}: export_csr differs"


@pytest.mark.parametrize("rung", [20, 22, 24])
def test_ladder_conversion_matches_lifted_oracle(pkg, oracle, ctx, rung):
    case, ref, gA, gB, _ = _rung(pkg, oracle, ctx, rung)
    _check_tiled(gA, ref.A, f"rung {rung} A")
    _check_tiled(gB, ref.B, f"rung {rung} A^T")
    assert pkg.flop_count(ctx, gA, gB) == oracle.flop_count(ref.oA, ref.oB)


@pytest.mark.parametrize("segments", [0, 1])
@pytest.mark.parametrize("xl_global", [0, 1])
@pytest.mark.parametrize("prune", [1, 0])
@pytest.mark.parametrize("rung", [20, 22, 24])
def test_ladder_three_steps_match_lifted_oracle(pkg, oracle, ctx, rung, prune, xl_global, segments):
    """a cold and a warm pass at each rung: counts, every plan array, both exports and the values against the lifted oracle, and
    the mix of 32-bit and 64-bit row sorts the rung stands for must be the one that ran"""
    case, ref, gA, gB, coo = _rung(pkg, oracle, ctx, rung)
    want_arrays, want_counts = expected(ref.op, ref.oA, ref.oB, bool(prune))
    plan = pkg.CPlan(ctx, gA, gB)
    for k, v in (("prune", prune), ("s1_xl_global", xl_global), ("s1_segments", segments), ("s3_poison", 1)):
        plan.set_option(k, v)
    must, never = _ladder_kernels(rung, segments, xl_global)
    for rnd in ("cold", "warm"):
        with _Profiled(ctx) as prof:
            plan.spgemm()
        label = f"rung {rung} prune={prune} xl_global={xl_global} segments={segments} {rnd}"
        assert must <= prof.names, f"{label}: did not run {sorted(must - prof.names)}"
        assert not (never & prof.names), f"{label}: ran {sorted(never & prof.names)}"
        _check_plan(plan, ref, want_arrays, want_counts, coo, label, csr=rung == 20)


def test_ladder_fp32_pass_at_rung_22(pkg, oracle, ctx):
    rung = 22
    case, ref, _, _, _ = _rung(pkg, oracle, ctx, rung)
    rows, cols, I, J, V, tr = case
    V32 = V.astype(np.float32)
    gA = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V32, False, dtype=np.float32)
    gB = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V32, True, dtype=np.float32)
    for g, lifted in ((gA, ref.A), (gB, ref.B)):
        _check_tiled(g, lifted, "rung 22 fp32", vals=lifted.o.vals.astype(np.float32))
    (r0, c0, v0), _ = ref.csr_spgemm_coo(f32=True, values=V32.astype(np.float64))
    want_arrays, want_counts = expected(ref.op, ref.oA, ref.oB, True)
    lifted = lift_plan_arrays(want_arrays, ref.rmap, ref.cmap, expand=False)
    plan = pkg.CPlan(ctx, gA, gB)
    plan.set_option("s3_poison", 1)
    must, never = _ladder_kernels(rung, 0, 0)
    for rnd in ("cold", "warm"):
        with _Profiled(ctx) as prof:
            plan.spgemm()
        assert must <= prof.names and not (never & prof.names), (rnd, sorted(prof.names))
        info = plan.info()
        assert (info["ntiles_c"], info["npairs"], info["nnz_c"], info["npairs_all"]) == want_counts
        for arr in C_NAMES:
            if arr == "c_tile_rowptr":
                assert ref.rmap.ptr_matches(plan.array(arr), lifted[arr]), arr
            elif arr != "c_vals":
                assert _same(plan.array(arr), lifted[arr]), f"fp32 {rnd}: plan array {arr} differs"
        r, c, v = plan.export_coo()
        assert _same(r, r0) and _same(c, c0)
        assert v.dtype == np.float32 and np.array_equal(v.astype(np.float64), v0), "fp32 values: the float fma chain bit for bit"
        assert not poisoned(plan.array("c_vals")).any()


@pytest.mark.parametrize("complement", [False, True])
def test_ladder_masked_pass_at_rung_22(pkg, oracle, ctx, complement):
    """mask = the product's own pattern, computed on the host: C<M> is all of C, and the complement keeps the C tiles that are not
    full and nothing in them"""
    rung = 22
    case, ref, gA, gB, coo = _rung(pkg, oracle, ctx, rung)
    rows = case[0]
    M = pkg.Tiled.from_coo(ctx, rows, rows, coo[0], coo[1], np.zeros(len(coo[0])))
    unmasked = pkg.CPlan(ctx, gA, gB)
    unmasked.spgemm()
    plan = pkg.CPlan(ctx, gA, gB, mask=M, complement=complement)
    must, never = _ladder_kernels(rung, 0, 0)
    with _Profiled(ctx) as prof:
        plan.spgemm()
    assert must <= prof.names and not (never & prof.names), sorted(prof.names)
    u = {k: unmasked.array(k) for k in ("c_tile_rowptr", "c_tile_colidx", "pairs_offset", "pairs_a", "pairs_b", "c_mask")}
    u["tr_lo"] = 0
    m = dict(tile_rowptr=M.array("tile_rowptr"), tile_colidx=M.array("tile_colidx"), masks=M.array("masks"), tile_cols=M.tile_cols)
    want = maskref.restate(u, m, complement)
    info = plan.info()
    assert (info["ntiles_c"], info["npairs"], info["nnz_c"]) == (want["ntiles_c"], want["npairs"], want["nnz_c"])
    assert info["npairs_all"] == unmasked.info()["npairs_all"]
    assert info["nnz_c"] == (0 if complement else len(coo[0]))
    for k in ("c_tile_rowptr", "c_tile_rowidx", "c_tile_colidx", "pairs_offset", "pairs_a", "pairs_b", "c_mask", "c_tile_nnz_ptr", "c_mtile",
              "c_rowcolidx"):
        assert _same(plan.array(k), want[k]), f"masked complement={complement}: {k}"
    r, c, v = plan.export_coo()
    keep = slice(0, 0) if complement else slice(None)
    assert _same(r, coo[0][keep]) and _same(c, coo[1][keep]) and _same(v, coo[2][keep])


# ------------------------------------------------------------------------------------------------------------------------------
# part 2: a hypersparse square tiling through every operation
# ------------------------------------------------------------------------------------------------------------------------------
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


def _past(plan):
    i = plan.info()
    assert min(i["tile_row_end"] - i["tile_row_begin"], i["ntiles_c"], i["nnz_c"]) > SCAN_CHAINED_MAX, "the product is not past the chained scan"


def test_hyper_conversions_match_lifted_oracle(pkg, oracle, tctx):
    H = _hyper(pkg, tctx, np.float64)
    n, I, J, V = H.n, H.I, H.J, H.V
    plain, transposed = (compactref.lifted_tiled(oracle, n, n, I, J, V, tr) for tr in (False, True))
    with _Profiled(tctx) as prof:
        fresh = pkg.Tiled.from_coo(tctx, n, n, I, J, V)
    assert "scan_reduce_kernel" in prof.names, "no scan of the conversion took the three-launch form"
    _check_tiled(fresh, plain, "hypersparse from_coo")
    _check_tiled(pkg.Tiled.from_coo(tctx, n, n, I, J, V, True), transposed, "hypersparse from_coo(transpose)")
    dI, dJ, dV = _dev(I), _dev(J), _dev(V)
    for tr, lifted in ((False, plain), (True, transposed)):
        g = pkg.Tiled.from_coo_device(tctx, n, n, len(I), dI.data_ptr(), dJ.data_ptr(), dV.data_ptr(), tr)
        _check_tiled(g, lifted, f"hypersparse from_coo_device(transpose={tr})")
    rp, ci, v = H.csr()
    _check_tiled(pkg.Tiled.from_csr(tctx, n, n, rp, ci, v), plain, "hypersparse from_csr")
    assert min(plain.tile_rows, plain.tile_cols, plain.ntiles) > SCAN_CHAINED_MAX


PRODUCT_OPTIONS = {"default": (), "prune0": (("prune", 0),), "class_scan0": (("s1_class_scan", 0),), "class_scan1": (("s1_class_scan", 1),),
                   "global_sort": (("step1_global_sort", 1),)}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("options", list(PRODUCT_OPTIONS))
def test_hyper_product_matches_lifted_serial_csr(pkg, oracle, tctx, options, dtype):
    H = _hyper(pkg, tctx, dtype)
    r0, c0, v0 = H.product(oracle)
    plan = pkg.CPlan(tctx, H.A, H.A)
    for k, v in PRODUCT_OPTIONS[options] + (("s3_poison", 1),):
        plan.set_option(k, v)
    for rnd in ("cold", "warm"):
        with _Profiled(tctx) as prof:
            plan.spgemm()
        assert "scan_reduce_kernel" in prof.names, f"{options} {rnd}: no scan took the three-launch form"
        if options != "global_sort":
            assert "s1_rowclass_kernel" in prof.names and "s1_rowclass_kernel<scan>" not in prof.names, sorted(prof.names)
        _past(plan)
        r, c, v = plan.export_coo()
        assert _same(r, r0) and _same(c, c0), f"{options} {rnd}: structure"
        assert _same(v, v0), f"{options} {rnd}: values must match the ascending-k fma chain bit for bit"
        rp, ci, cv = plan.export_csr()
        assert _same(ci, c0) and _same(cv, v0) and np.array_equal(np.repeat(np.arange(H.n, dtype=np.int32), np.diff(rp)), r0)


@pytest.mark.parametrize("complement", [False, True])
def test_hyper_masked_product(pkg, oracle, tctx, complement):
    H = _hyper(pkg, tctx, np.float64)
    n = H.n
    r0, c0, v0 = H.product(oracle)
    unmasked = pkg.CPlan(tctx, H.A, H.A)
    unmasked.spgemm()
    plan = pkg.CPlan(tctx, H.A, H.A, mask=H.A, complement=complement)
    plan.spgemm()
    u = {k: unmasked.array(k) for k in ("c_tile_rowptr", "c_tile_colidx", "pairs_offset", "pairs_a", "pairs_b", "c_mask")}
    u["tr_lo"] = 0
    m = dict(tile_rowptr=H.A.array("tile_rowptr"), tile_colidx=H.A.array("tile_colidx"), masks=H.A.array("masks"), tile_cols=H.A.tile_cols)
    want = maskref.restate(u, m, complement)
    info = plan.info()
    assert (info["ntiles_c"], info["npairs"], info["nnz_c"]) == (want["ntiles_c"], want["npairs"], want["nnz_c"])
    assert info["tile_row_end"] - info["tile_row_begin"] > SCAN_CHAINED_MAX
    for k in ("c_tile_rowptr", "c_tile_rowidx", "c_tile_colidx", "pairs_offset", "pairs_a", "pairs_b", "c_mask", "c_tile_nnz_ptr", "c_mtile",
              "c_rowcolidx"):
        assert _same(plan.array(k), want[k]), f"masked complement={complement}: {k}"
    keep = np.isin(maskref.pattern_keys(r0, c0, n), maskref.pattern_keys(H.I, H.J, n)) != complement
    assert 0 < keep.sum() < len(keep)
    r, c, v = plan.export_coo()
    assert _same(r, r0[keep]) and _same(c, c0[keep]) and _same(v, v0[keep])


@pytest.mark.parametrize("semiring", ["min_plus", "plus_pair"])
def test_hyper_semirings(pkg, tctx, semiring):
    H = _hyper(pkg, tctx, np.float64)
    plan = pkg.CPlan(tctx, H.A, H.A, semiring=semiring)
    plan.spgemm()
    _past(plan)
    # semiringref on the used lines (its row loop and row pointer are as long as the dimension), lifted through the same map
    m = H.map
    wrp, wci, wv = sr.spgemm(H.ccsr, H.ccsr, m.cdim, semiring)
    wr = m.used[np.repeat(np.arange(m.cdim, dtype=np.int64), np.diff(wrp))].astype(np.int32)
    r, c, v = plan.export_coo()
    assert np.array_equal(r, wr) and np.array_equal(c, m.used[wci].astype(np.int32)), f"{semiring}: structure"
    assert v.dtype == wv.dtype and sr.same_values(v, wv), f"{semiring}: values"


def test_hyper_set_values_and_step3_refresh(pkg, oracle, tctx):
    H = _hyper(pkg, tctx, np.float64)
    A = pkg.Tiled.from_coo(tctx, H.n, H.n, H.I, H.J, H.V)
    plan = pkg.CPlan(tctx, A, A)
    plan.spgemm()
    rng = np.random.default_rng(31)
    W = rng.uniform(-2.0, 2.0, len(H.V))                 # new values, in the case's entry order
    order = np.argsort(H.I.astype(np.int64) * H.n + H.J, kind="stable")
    A.set_values(W[order], "row")
    plan.step3()
    r0, c0, v0 = H.product(oracle, W)
    r, c, v = plan.export_coo()
    assert _same(r, r0) and _same(c, c0) and _same(v, v0)
    assert _same(A.array("vals"), compactref.lifted_tiled(oracle, H.n, H.n, H.I, H.J, W).array("vals"))


def test_hyper_chain(pkg, oracle, tctx):
    H = _hyper(pkg, tctx, np.float64)
    n = H.n
    plan = pkg.CPlan(tctx, H.A, H.A)
    plan.spgemm()
    r0, c0, v0 = H.product(oracle)
    for tr in (0, 1):
        got = pkg.Tiled.from_cplan(plan, transpose=tr)
        want = pkg.Tiled.from_coo(tctx, n, n, r0, c0, v0, bool(tr))        # (the reconversion of test_gpu_chain.py, from the oracle's C)
        _assert_same_tiling(got, want, f"from_cplan transpose={tr}")
        pay = chainref.brute_force(r0, c0, v0, transpose=bool(tr))
        for k in ("tile_keys", "tile_nnz_ptr", "rowcolidx", "vals"):
            assert _same(got.array(k), pay[k]), f"from_cplan transpose={tr}: {k} differs from chainref"
    Ct = pkg.Tiled.from_cplan(plan)
    second = pkg.CPlan(tctx, Ct, H.A)                      # (A*A)*A against the oracle applied twice
    second.spgemm()
    _past(second)
    w = compactref.product_coo(oracle, n, (r0, c0, v0), (H.I, H.J, H.V))
    for got, want in zip(second.export_coo(), w):
        assert _same(got, want)
    W = np.random.default_rng(37).uniform(-2.0, 2.0, len(H.V))
    A2 = pkg.Tiled.from_coo(tctx, n, n, H.I, H.J, H.V)
    p2 = pkg.CPlan(tctx, A2, A2)
    p2.spgemm()
    T = pkg.Tiled.from_cplan(p2, transpose=1)
    A2.set_values(W[np.argsort(H.I.astype(np.int64) * n + H.J, kind="stable")], "row")
    p2.step3()
    T.set_values_from_cplan(p2)
    _assert_same_tiling(T, pkg.Tiled.from_coo(tctx, n, n, *H.product(oracle, W), True), "set_values_from_cplan")


def test_hyper_ewise_and_refresh(pkg, tctx):
    H = _hyper(pkg, tctx, np.float64)
    n = H.n
    B = pkg.Tiled.from_coo(tctx, n, n, H.I, H.J, H.V, True)               # A^T: shares the clique's symmetric part and the dense tile
    b = _canonical(H.J, H.I, H.V, n)
    for op, pattern, alpha, beta in (("plus", "union", 2.0, -0.5), ("times", "intersect", 0.25, 3.0)):
        R = pkg.Tiled.ewise(H.A, B, op=op, pattern=pattern, alpha=alpha, beta=beta)
        wI, wJ, wV = ew.ewise(n, H.coo, b, op, pattern, alpha, beta)
        assert 0 < len(wI) and (pattern == "intersect" or len(wI) > len(H.I))
        _assert_same_tiling(R, pkg.Tiled.from_coo(tctx, n, n, wI, wJ, wV), f"ewise {op} {pattern}", past=pattern == "union")
    A2 = pkg.Tiled.from_coo(tctx, n, n, H.I, H.J, H.V)
    R = pkg.Tiled.ewise(A2, B, op="plus", pattern="union", alpha=2.0, beta=-0.5)
    W = np.random.default_rng(41).uniform(-2.0, 2.0, len(H.V))
    a2 = _canonical(H.I, H.J, W, n)
    A2.set_values(a2[2], "row")
    R.set_values_from_ewise(A2, B)
    wI, wJ, wV = ew.ewise(n, a2, b, "plus", "union", 2.0, -0.5)
    _assert_same_tiling(R, pkg.Tiled.from_coo(tctx, n, n, wI, wJ, wV), "set_values_from_ewise")


@pytest.mark.parametrize("op,thunk", [("tril", 4_194_304), ("tril", -4_194_304), ("triu", 4_194_304), ("triu", -4_194_304),
                                      ("diag", 0), ("diag", 4_194_304), ("offdiag", -4_194_304), ("offdiag", 0), ("abs_gt", 0.5)])
def test_hyper_select(pkg, tctx, op, thunk):
    """thunks of +-4 194 304 = 2^22: i - j leaves 22 bits, and the clique holds entries on both of those diagonals' sides"""
    H = _hyper(pkg, tctx, np.float64)
    wI, wJ, wV = sel.select(*H.coo, op, thunk)
    assert 0 < len(wI) < len(H.I) or op == "offdiag", (op, thunk, len(wI))
    R = H.A.select(op, thunk)
    _assert_same_tiling(R, pkg.Tiled.from_coo(tctx, H.n, H.n, wI, wJ, wV), f"select {op} {thunk}", past=False)
    assert R.tile_rows > SCAN_CHAINED_MAX


def _lists(H):
    """index lists that cross tile row 262 144: a reversed range around it, one with repeats, and a subset of the clique set"""
    e = 16 * 262_144
    rng = np.random.default_rng(43)
    rev = np.arange(e - 40, e + 21)[::-1]
    rep = np.concatenate([rng.integers(e - 64, e + 21, 300), H.S[rng.integers(0, len(H.S), 500)], rng.choice(H.I, 2000)])
    sub = H.S[::2]
    return {"reversed": (rev, rev), "repeats": (rep, np.concatenate([rep[::-1], H.S])), "subset": (sub, H.S)}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_hyper_transpose_and_refresh(pkg, tctx, dtype):
    H = _hyper(pkg, tctx, dtype)
    n = H.n
    A = pkg.Tiled.from_coo(tctx, n, n, H.I, H.J, H.V, dtype=dtype)
    T = A.transpose()
    _assert_same_tiling(T, pkg.Tiled.from_coo(tctx, n, n, H.I, H.J, H.V, True, dtype=dtype), "transpose")
    _assert_same_tiling(T.transpose(), A, "transpose twice")
    W = np.random.default_rng(47).uniform(-2.0, 2.0, len(H.V)).astype(dtype)
    A.set_values(_canonical(H.I, H.J, W, n)[2], "row")
    T.set_values_from_transpose(A)
    _assert_same_tiling(T, pkg.Tiled.from_coo(tctx, n, n, H.I, H.J, W, True, dtype=dtype), "set_values_from_transpose")


def test_hyper_extract_and_refresh(pkg, tctx):
    H = _hyper(pkg, tctx, np.float64)
    n = H.n
    A = pkg.Tiled.from_coo(tctx, n, n, H.I, H.J, H.V)
    W = np.random.default_rng(53).uniform(-2.0, 2.0, len(H.V))
    made = {}
    for kind, (RI, CJ) in _lists(H).items():
        ni, nj, wi, wj, wv = ex.extract(n, n, *H.coo, RI, CJ)
        assert len(wi) > 0, kind
        R = A.extract(RI, CJ)
        _assert_same_tiling(R, pkg.Tiled.from_coo(tctx, ni, nj, wi, wj, wv), f"extract {kind}", past=False)
        _assert_same_tiling(A.extract(_dev(RI.astype(np.int32)), _dev(CJ.astype(np.int32))), R, f"extract {kind} device lists", past=False)
        made[kind] = R
    rows_only = A.extract(np.arange(n - 1, -1, -1), None)                   # every row, reversed: the result keeps every dimension
    ni, nj, wi, wj, wv = ex.extract(n, n, *H.coo, np.arange(n - 1, -1, -1), None)
    _assert_same_tiling(rows_only, pkg.Tiled.from_coo(tctx, ni, nj, wi, wj, wv), "extract all rows reversed")
    a2 = _canonical(H.I, H.J, W, n)
    A.set_values(a2[2], "row")
    for kind, (RI, CJ) in _lists(H).items():
        ni, nj, wi, wj, wv = ex.extract(n, n, *a2, RI, CJ)
        made[kind].set_values_from_extract(A)
        _assert_same_tiling(made[kind], pkg.Tiled.from_coo(tctx, ni, nj, wi, wj, wv), f"set_values_from_extract {kind}", past=False)


@pytest.mark.parametrize("accum", [None, "plus"])
def test_hyper_assign_and_refresh(pkg, tctx, accum):
    H = _hyper(pkg, tctx, np.float64)
    n = H.n
    rng = np.random.default_rng(59)
    e = 16 * 262_144
    RI = np.unique(np.concatenate([H.S[::2], np.arange(e - 24, e + 21)]))[::-1].copy()      # no repeats; any order
    CJ = np.unique(np.concatenate([H.S, np.arange(e - 8, e + 21)]))
    k = rng.choice(len(RI) * len(CJ), 9000, replace=False)
    a = _canonical((k // len(CJ)).astype(np.int32), (k % len(CJ)).astype(np.int32), rng.uniform(-1.0, 1.0, len(k)), len(CJ))
    C = pkg.Tiled.from_coo(tctx, n, n, H.I, H.J, H.V)
    S = pkg.Tiled.from_coo(tctx, len(RI), len(CJ), *a)
    Z = C.assign(S, RI, CJ, accum=accum)
    wI, wJ, wV = asg.assign(n, n, H.coo, a, RI, CJ, accum)
    assert len(wI) != len(H.I)
    _assert_same_tiling(Z, pkg.Tiled.from_coo(tctx, n, n, wI, wJ, wV), f"assign accum={accum}")
    _assert_same_tiling(C.assign(S, _dev(RI.astype(np.int32)), _dev(CJ.astype(np.int32)), accum=accum), Z, "assign, device lists")
    W = rng.uniform(-2.0, 2.0, len(H.V))
    c2 = _canonical(H.I, H.J, W, n)
    C.set_values(c2[2], "row")
    Z.set_values_from_assign(C, S)
    wI, wJ, wV = asg.assign(n, n, c2, a, RI, CJ, accum)
    _assert_same_tiling(Z, pkg.Tiled.from_coo(tctx, n, n, wI, wJ, wV), f"set_values_from_assign accum={accum}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("tr", [False, True], ids=("Ax", "ATx"))
def test_hyper_mxv(pkg, oracle, tctx, tr, dtype):
    """every semiring, both directions, accumulate on and off, against mxvref on the used lines"""
    H = _hyper(pkg, tctx, dtype)
    n, m = H.n, H.map
    rng = np.random.default_rng(61)
    x, y0 = rng.standard_normal(n).astype(dtype), rng.standard_normal(n).astype(dtype)
    dx = _dev(x)
    xc, yc = m.gather(x), m.gather(y0)
    for s in mr.SEMIRINGS:
        want = m.scatter(mr.mxv(m.cdim, m.cdim, *H.ccsr, xc, s, dtype, oracle=oracle, transpose=tr), mr.MXV_START[s])
        assert _same_vec(_host(H.A.mxv(dx, s, transpose=tr)), want, s), f"mxv {s} transpose={tr}"
        out = _dev(y0)
        assert H.A.mxv(dx, s, transpose=tr, out=out, accumulate=True) is out
        want = m.scatter(mr.mxv(m.cdim, m.cdim, *H.ccsr, xc, s, dtype, y0=yc, oracle=oracle, transpose=tr), y0)
        assert _same_vec(_host(out), want, s), f"mxv {s} transpose={tr} accumulate"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("dim", ["rows", "cols"])
def test_hyper_reduce(pkg, tctx, dim, dtype):
    H = _hyper(pkg, tctx, dtype)
    n, m = H.n, H.map
    y0 = np.random.default_rng(63).standard_normal(n).astype(dtype)
    yc = m.gather(y0)
    for op in mr.OPS:
        want = m.scatter(mr.reduce(m.cdim, m.cdim, *H.ccsr, op, dtype, dim=dim), mr.IDENTITY[op])
        assert _same_vec(_host(H.A.reduce(op, dim)), want, op), f"reduce {op} {dim}"
        out = _dev(y0)
        H.A.reduce(op, dim, out=out, accumulate=True)
        want = m.scatter(mr.reduce(m.cdim, m.cdim, *H.ccsr, op, dtype, y0=yc, dim=dim), y0)
        assert _same_vec(_host(out), want, op), f"reduce {op} {dim} accumulate"


@pytest.mark.parametrize("transpose", [False, True])
def test_hyper_frontier(pkg, oracle, tctx, transpose):
    """a 1 000-entry x_present, an output mask and its complement; the line flags of the call against frontierref's mark rule"""
    H = _hyper(pkg, tctx, np.float64)
    n, m = H.n, H.map
    rng = np.random.default_rng(67)
    x, y_old = rng.standard_normal(n), rng.standard_normal(n)
    present = np.zeros(n, np.uint8)
    present[np.concatenate([rng.choice(m.used, 900, replace=False), H.S[:60], rng.integers(0, n, 40)])] = 1
    present[np.flatnonzero(present)[1000:]] = 0
    assert present.sum() == 1000
    mask = (rng.random(n) < 0.5).astype(np.uint8)
    dx, dp, dm = _dev(x), _dev(present), _dev(mask)
    rp, ci, v = H.csr()
    for s in ("plus_times", "min_plus", "plus_pair"):
        for comp in (False, True):
            for acc in (False, True):
                yc, pc = fr.mxv_frontier(m.cdim, m.cdim, *H.ccsr, m.gather(x), s, np.float64, present=m.gather(present),
                                         y_old=m.gather(y_old) if acc else None, accumulate=acc, oracle=oracle, transpose=transpose)
                allowed = fr.allowed_of(n, mask, comp)
                res = m.scatter(yc, y_old if acc else mr.MXV_START[s])
                want_y = np.where(allowed, res, y_old)
                want_p = (allowed & (m.scatter(pc, 0) != 0)).astype(np.uint8)
                out, op = _dev(y_old), torch.zeros(n, dtype=torch.uint8, device="cuda")
                H.A.mxv_frontier(dx, dp, dm, comp, s, transpose, out=out, accumulate=acc, out_present=op)
                assert _same_vec(_host(out), want_y, s), f"frontier {s} complement={comp} accumulate={acc}"
                assert np.array_equal(_host(op), want_p) and 0 < want_p.sum() < 16 * 1000
        flags = H.A.frontier_line_flags(transpose)
        assert np.array_equal(flags, fr.line_flags(n, n, rp, ci, present, transpose)) and 0 < flags.sum() < len(flags)


@pytest.mark.parametrize("source", [0, HYPER_N - 1])
def test_hyper_bfs(pkg, tctx, source):
    H = _hyper(pkg, tctx, np.float64)
    rp, ci, _ = H.csr()
    for tr in (False, True):
        want, depth, reached = fr.bfs(H.n, rp, ci, source, tr)
        levels, d, r = H.A.bfs(source, tr)
        assert (d, r) == (depth, reached) and reached > 400 and depth >= 2, (source, tr, depth, reached)
        assert np.array_equal(_host(levels), want)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("k", [3, 6, 9])
def test_hyper_spmm(pkg, oracle, tctx, k, dtype):
    """the three widths, X and Y column slices of wider row-major arrays; columns of Y past k are never written"""
    H = _hyper(pkg, tctx, dtype)
    n, m = H.n, H.map
    rng = np.random.default_rng(71 + k)
    Xw, Yw = rng.standard_normal((n, k + 2)).astype(dtype), rng.standard_normal((n, k + 3)).astype(dtype)
    Xc = np.ascontiguousarray(Xw[m.used, :k])
    for s, tr, acc in (("plus_times", False, False), ("plus_times", True, True), ("min_plus", False, True), ("max_times", True, False)):
        dX, dY = _dev(Xw), _dev(Yw)
        H.A.spmm(dX[:, :k], s, tr, out=dY[:, :k], accumulate=acc)
        Yc = sp.spmm(m.cdim, m.cdim, *H.ccsr, Xc, s, dtype, Y0=np.ascontiguousarray(Yw[m.used, :k]) if acc else None, oracle=oracle, transpose=tr)
        want = Yw.copy()
        want[:, :k] = Yw[:, :k] if acc else mr.MXV_START[s]
        want[m.used, :k] = Yc
        assert _same_vec(_host(dY), want, s), f"spmm k={k} {s} transpose={tr} accumulate={acc}"


def test_hyper_sddmm(pkg, oracle, tctx):
    H = _hyper(pkg, tctx, np.float64)
    n, k = H.n, 4
    rng = np.random.default_rng(73)
    I, J = H.coo[0], H.coo[1]
    rows_used, cols_used = np.unique(I), np.unique(J)
    X, Y = np.zeros((n, k)), np.zeros((n, k))                              # (only the lines with entries are read)
    X[rows_used], Y[cols_used] = rng.standard_normal((len(rows_used), k)), rng.standard_normal((len(cols_used), k))
    dX, dY = _dev(X), _dev(Y)
    for s in ("plus_times", "min_plus"):
        R = H.A.sddmm(dX, dY, s)
        want = sd.sddmm(I, J, X, Y, s, np.float64, oracle=oracle)
        _assert_same_tiling(R, pkg.Tiled.from_coo(tctx, n, n, I, J, want), f"sddmm {s}")
    A2 = pkg.Tiled.from_coo(tctx, n, n, H.I, H.J, H.V)
    for s, acc in (("plus_times", True), ("max_plus", False)):
        old = A2.export_csr()[2]
        A2.set_values_sddmm(dX, dY, s, accumulate=acc)
        want = sd.sddmm(I, J, X, Y, s, np.float64, old=old if acc else None, oracle=oracle)
        _assert_same_tiling(A2, pkg.Tiled.from_coo(tctx, n, n, I, J, want), f"set_values_sddmm {s} accumulate={acc}")


def test_hyper_save_load_round_trip(pkg, tctx, tmp_path):
    H = _hyper(pkg, tctx, np.float64)
    path = str(tmp_path / "hyper.pemt")
    H.A.save(path)
    _assert_same_tiling(pkg.Tiled.load(tctx, path), H.A, "save / load")


# ------------------------------------------------------------------------------------------------------------------------------
# part 3: a conversion of more than 4 194 304 entries
# ------------------------------------------------------------------------------------------------------------------------------
DENSE_N = 2080
_DENSE = {}


def _dense(oracle):
    if not _DENSE:
        n = DENSE_N
        rng = np.random.default_rng(79)
        p = rng.permutation(n * n)
        I, J = (p // n).astype(np.int32), (p % n).astype(np.int32)
        V = rng.uniform(-1.0, 1.0, n * n)
        V[V == 0.0] = 0.25
        _DENSE.update(I=I, J=J, V=V, order=np.lexsort((J, I)), x=rng.standard_normal(n))
    return _DENSE


def _dense_tiled(oracle, transpose):
    D = _dense(oracle)
    if ("o", transpose) not in D:
        D["o", transpose] = oracle.Tiled(DENSE_N, DENSE_N, D["I"], D["J"], D["V"], transpose)
    return D["o", transpose]


def _dense_mxv(oracle, dtype, transpose):
    """A x (transpose: A^T x) of the dense matrix itself, shared by the tilings of A and of A^T"""
    D = _dense(oracle)
    key = ("y", np.dtype(dtype).name, transpose)
    if key not in D:
        n, o = DENSE_N, D["order"]
        csr = (np.arange(n + 1, dtype=np.int64) * n, D["J"][o].astype(np.int64), D["V"].astype(dtype)[o])
        D[key] = mr.mxv(n, n, *csr, D["x"].astype(dtype), "plus_times", dtype, oracle=oracle, transpose=transpose)
    return D[key]


@pytest.mark.parametrize("transpose", [False, True], ids=("plain", "transposed"))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_dense_conversion_past_1024_sort_blocks(pkg, oracle, tctx, dtype, transpose):
    n = DENSE_N
    D = _dense(oracle)
    I, J, V, o = D["I"], D["J"], D["V"].astype(dtype), _dense_tiled(oracle, transpose)
    assert len(I) > 4_194_304 and -(-len(I) // SORT_BLOCK_KEYS) > 1024
    with _Profiled(tctx) as prof:
        g = pkg.Tiled.from_coo(tctx, n, n, I, J, V, transpose, dtype=dtype)
    # The conversion scans in three launches: the histogram of every pass of the entry sort (8 in-tile bits + the bits of 130 tile
    # rows and of 130 tile columns = 24 bits, three passes of 8; 256 words per block, 1057 blocks) and the tile heads, one per entry.
    # Below 1025 blocks only the head scan does; the second sort, of the 16 900 tiles, has a histogram of five blocks.
    tile_bits = int(np.ceil(np.log2(-(-n // 16))))
    passes = -(-(8 + 2 * tile_bits) // 8)
    assert prof.stats["rs_hist_kernel"]["calls"] == passes + 1, prof.stats["rs_hist_kernel"]
    assert prof.stats["scan_reduce_kernel"]["calls"] >= passes + 1, \
        f"the sort's histogram scans did not take the three-launch form: {prof.stats['scan_reduce_kernel']['calls']} such scans"
    assert (g.rows, g.cols, g.nnz, g.tile_rows, g.tile_cols, g.ntiles) == (o.rows, o.cols, o.nnz, o.tile_rows, o.tile_cols, o.ntiles)
    for arr in T_NAMES:
        want = getattr(o, arr).astype(dtype) if arr == "vals" else getattr(o, arr)
        assert _same(g.array(arr), want), f"dense {arr} differs"
    ti, tj = (J, I) if transpose else (I, J)
    order = np.lexsort((tj, ti))                                           # conversion does no arithmetic: the entries, sorted
    rp, ci, v = g.export_csr()
    assert np.array_equal(rp, np.arange(n + 1, dtype=np.int32) * n) and np.array_equal(ci, tj[order]) and _same(v, V[order])
    dx = _dev(D["x"].astype(dtype))
    for tr in (False, True):                                               # (the tiling of A^T times x is A^T x of the matrix itself)
        assert _same_vec(_host(g.mxv(dx, "plus_times", transpose=tr)), _dense_mxv(oracle, dtype, tr != transpose)), f"dense mxv transpose={tr}"
