"""GPU: masked products C<M> = A*B (pem_cplan_create_masked, CPlan(..., mask=M, complement=...)).

Every masked plan is held to two things: its arrays equal the numpy restatement of the filter and the AND (tests/maskref.py)
applied to the device's UNMASKED plan on the same options, bit for bit; and its exports equal the oracle's C filtered by M --
structure exact, values bit-exact.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import maskref
from matgen import _vals, cases
from s3cases import poisoned

pytestmark = pytest.mark.gpu

torch.cuda.is_available()   # (torch's runtime first, as in test_gpu_values.py)

CASES = cases()
PEM_E_INVALID = -1
ARRAYS = ("c_tile_rowptr", "c_tile_rowidx", "c_tile_colidx", "pairs_offset", "pairs_a", "pairs_b", "c_mask", "c_tile_nnz_ptr", "c_mtile",
          "c_rowcolidx")


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32) if a.dtype.kind == "f" else a


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _plan_arrays(plan):
    out = {k: plan.array(k) for k in ("c_tile_rowptr", "c_tile_colidx", "pairs_offset", "pairs_a", "pairs_b", "c_mask")}
    out["tr_lo"] = plan.info()["tile_row_begin"]
    return out


def _m_arrays(M):
    return dict(tile_rowptr=M.array("tile_rowptr"), tile_colidx=M.array("tile_colidx"), masks=M.array("masks"), tile_cols=M.tile_cols)


def _results(plan):
    return [*plan.export_csr(), *plan.export_coo(), plan.array("c_vals")]


def _tilings(pkg, ctx, case, dtype=np.float64, V=None):
    rows, cols, I, J, V0, tr = case
    V = V0 if V is None else V
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=dtype)
    B = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, True, dtype=dtype) if tr else A
    return A, B


def _csr_keys(rp, ci, ncols, row0=0):
    r = row0 + np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))
    return r * ncols + np.asarray(ci, np.int64)


def _mask_patterns(rng, rows, nc, c_rp, c_ci, square_a=None):
    """name -> (I, J) of masks of C's shape: empty, sparse random, dense tiles, partial tiles, A's pattern, unmasked C's pattern"""
    out = {"empty": (np.zeros(0, np.int32), np.zeros(0, np.int32))}
    total = rows * nc
    nz = int(min(max(total // 50, 1), 20000))
    key = np.unique(rng.integers(0, total, nz, dtype=np.int64))
    out["sparse"] = ((key // nc).astype(np.int32), (key % nc).astype(np.int32))
    ckey = _csr_keys(c_rp, c_ci, nc)
    ctiles = np.unique((ckey // nc // 16) * ((nc + 15) // 16) + (ckey % nc) // 16)
    pick = rng.choice(ctiles, min(len(ctiles), 40), replace=False) if len(ctiles) else ctiles
    ti, tj = pick // ((nc + 15) // 16), pick % ((nc + 15) // 16)
    rr, cc = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    I = (16 * ti[:, None] + rr.ravel()[None, :]).ravel()
    J = (16 * tj[:, None] + cc.ravel()[None, :]).ravel()
    ok = (I < rows) & (J < nc)
    out["dense_tiles"] = (I[ok].astype(np.int32), J[ok].astype(np.int32))
    half = ckey[rng.random(len(ckey)) < 0.5]
    pk = np.unique(np.concatenate([half, key[: len(key) // 2]]))
    out["partial"] = ((pk // nc).astype(np.int32), (pk % nc).astype(np.int32))
    if square_a is not None:
        out["A"] = square_a
    out["C"] = ((ckey // nc).astype(np.int32), (ckey % nc).astype(np.int32))
    return out


def _check_masked(pkg, ctx, A, B, M, MI, MJ, complement, unmasked, c_full, options=(), label=""):
    """masked plan on (A, B, M) against the restatement of `unmasked` (same options, pass done) and the filtered C `c_full`"""
    nc = B.cols
    plan = pkg.CPlan(ctx, A, B, mask=M, complement=complement)
    for k, v in options:
        plan.set_option(k, v)
    plan.spgemm()
    want = maskref.restate(_plan_arrays(unmasked), _m_arrays(M), complement)
    info, uinfo = plan.info(), unmasked.info()
    assert (info["ntiles_c"], info["npairs"], info["nnz_c"]) == (want["ntiles_c"], want["npairs"], want["nnz_c"]), label
    assert info["npairs_all"] == uinfo["npairs_all"], label
    for k in ARRAYS:
        assert _same(plan.array(k), want[k]), f"{label}: {k}"
    rp, ci, v = plan.export_csr()
    frp, fci, fv = maskref.filter_csr(*c_full, MI, MJ, nc, complement)
    assert _same(rp, frp) and _same(ci, fci) and _same(v, fv), f"{label}: CSR export"
    r, c, cv = plan.export_coo()
    order = np.lexsort((c, r))
    assert _same(_csr_keys(rp, ci, nc), r[order].astype(np.int64) * nc + c[order]) and _same(cv[order], v), f"{label}: COO export"
    return plan


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case_every_mask(pkg, oracle, ctx, name):
    rows, cols, I, J, V, tr = case = CASES[name]
    A, B = _tilings(pkg, ctx, case)
    nc = B.cols
    unmasked = pkg.CPlan(ctx, A, B)
    unmasked.spgemm()
    oa = oracle.Csr(rows, cols, I, J, V)
    ob = oracle.Csr(rows, cols, I, J, V, tr) if tr else oa
    c_full = oracle.csr_spgemm(oa, ob).arrays()
    assert all(_same(g, w) for g, w in zip(unmasked.export_csr(), c_full))
    rng = np.random.default_rng(len(name) * 1000 + rows)
    for mname, (MI, MJ) in _mask_patterns(rng, rows, nc, *c_full[:2], square_a=(I, J) if rows == cols and not tr else None).items():
        M = pkg.Tiled.from_coo(ctx, rows, nc, MI, MJ, np.zeros(len(MI)))
        for comp in (False, True):
            _check_masked(pkg, ctx, A, B, M, MI, MJ, comp, unmasked, c_full, label=f"{name} {mname} complement={comp}")


def test_identities(pkg, oracle, ctx):
    rows, cols, I, J, V, tr = case = CASES["powerlaw_600"]
    A, B = _tilings(pkg, ctx, case)
    full = pkg.CPlan(ctx, A, B)
    full.spgemm()
    want = _results(full)
    empty = pkg.Tiled.from_coo(ctx, rows, cols, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    p = pkg.CPlan(ctx, A, B, mask=empty, complement=True)           # complement of nothing: all of C
    p.spgemm()
    assert all(_same(g, w) for g, w in zip(_results(p), want))
    rp, ci, _ = full.export_csr()
    r = np.repeat(np.arange(rows), np.diff(rp))
    Cpat = pkg.Tiled.from_coo(ctx, rows, cols, r, ci, np.ones(len(ci)))
    p = pkg.CPlan(ctx, A, B, mask=Cpat)                             # C's own pattern: all of C
    p.spgemm()
    assert all(_same(g, w) for g, w in zip(_results(p), want))
    for k in ("c_tile_rowptr", "c_tile_colidx", "pairs_offset", "pairs_a", "pairs_b", "c_mask", "c_tile_nnz_ptr"):
        assert _same(p.array(k), full.array(k)), k
    p = pkg.CPlan(ctx, A, B, mask=empty)                            # nothing
    p.spgemm()
    assert p.info()["nnz_c"] == 0 and p.info()["ntiles_c"] == 0
    rp0, ci0, v0 = p.export_csr()
    assert len(rp0) == rows + 1 and not rp0.any() and len(ci0) == 0 and len(v0) == 0 and len(p.export_coo()[0]) == 0
    dI, dJ = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    dense = pkg.Tiled.from_coo(ctx, rows, cols, dI.ravel(), dJ.ravel(), np.zeros(dI.size))
    p = pkg.CPlan(ctx, A, B, mask=dense, complement=True)           # complement of everything: nothing
    p.spgemm()
    assert p.info()["nnz_c"] == 0
    assert not p.export_csr()[0].any()


OPTION_SETS = [(("prune", 0),), (("s2_transposed", 0),), (("s2_transposed", 1),), (("s2_transposed", 2),), (("s3_decode", 0),),
               (("s3_band", 0),), (("s3_mark", 0),), (("warm", 0),)]


@pytest.mark.parametrize("name", ["rand_300", "band_1500", "dense_48", "banded_500_AAt", "hub_row_4000", "blockrows_1600"])
@pytest.mark.parametrize("options", OPTION_SETS, ids=lambda o: "-".join(f"{k}{v}" for k, v in o))
def test_options(pkg, oracle, ctx, name, options):
    rows, cols, I, J, V, tr = case = CASES[name]
    A, B = _tilings(pkg, ctx, case)
    unmasked = pkg.CPlan(ctx, A, B)
    for k, v in options:
        unmasked.set_option(k, v)
    unmasked.spgemm()
    unmasked.spgemm()                                             # (s2_transposed 2 takes effect on repeat passes)
    c_full = unmasked.export_csr()
    rng = np.random.default_rng(9)
    masks = _mask_patterns(rng, rows, B.cols, *c_full[:2], square_a=(I, J) if not tr else None)
    for mname in ("partial", "dense_tiles", "A" if not tr else "C"):
        MI, MJ = masks[mname]
        M = pkg.Tiled.from_coo(ctx, rows, B.cols, MI, MJ, np.ones(len(MI)))
        for comp in (False, True):
            plan = _check_masked(pkg, ctx, A, B, M, MI, MJ, comp, unmasked, c_full, options, f"{name} {options} {mname} {comp}")
            first = _results(plan)
            plan.spgemm()                                         # repeat pass (warm unless warm=0) on the same options
            assert all(_same(g, w) for g, w in zip(_results(plan), first)), f"{name} {options} {mname} repeat"


def test_fp32_operands_fp32_mask_and_mask_is_a(pkg, oracle, ctx):
    rows, cols, I, J, V, tr = case = CASES["rand_300"]
    for dtype in (np.float32, np.float64):
        A, B = _tilings(pkg, ctx, case, dtype)
        unmasked = pkg.CPlan(ctx, A, B)
        unmasked.spgemm()
        c_full = unmasked.export_csr()
        for m_dtype in (np.float32, np.float64):
            M = pkg.Tiled.from_coo(ctx, rows, cols, I, J, np.ones(len(I)), dtype=m_dtype)
            for comp in (False, True):
                _check_masked(pkg, ctx, A, B, M, I, J, comp, unmasked, c_full, label=f"{dtype} mask {m_dtype} {comp}")
        for comp in (False, True):                                 # M is A itself
            _check_masked(pkg, ctx, A, A, A, I, J, comp, unmasked, c_full, label=f"{dtype} M is A {comp}")


def test_stepwise_repeat_and_graph_replay(pkg, oracle, ctx):
    for name in ("rand_300", "band_1500", "banded_500_AAt"):
        rows, cols, I, J, V, tr = case = CASES[name]
        A, B = _tilings(pkg, ctx, case)
        M = pkg.Tiled.from_coo(ctx, rows, B.cols, I, J, V) if not tr else None
        if tr:
            u = pkg.CPlan(ctx, A, B)
            u.spgemm()
            rp, ci, _ = u.export_csr()
            keep = np.random.default_rng(2).random(len(ci)) < 0.4
            r = np.repeat(np.arange(rows), np.diff(rp))
            M = pkg.Tiled.from_coo(ctx, rows, B.cols, r[keep], ci[keep], np.ones(int(keep.sum())))
        for comp in (False, True):
            ref = pkg.CPlan(ctx, A, B, mask=M, complement=comp)
            ref.spgemm()
            want = _results(ref)
            want_arrays = {k: ref.array(k) for k in ARRAYS}
            ref.set_option("s3_poison", 1)                     # from here C holds a NaN fill before every step 3
            sw = pkg.CPlan(ctx, A, B, mask=M, complement=comp)
            sw.set_option("s3_poison", 1)
            sw.step1()
            for k in ("c_tile_rowptr", "c_tile_colidx", "pairs_offset", "c_mtile"):
                assert _same(sw.array(k), want_arrays[k]), f"{name} step 1 {k}"
            sw.step2()
            for k in ("pairs_a", "pairs_b", "c_mask", "c_tile_nnz_ptr"):
                assert _same(sw.array(k), want_arrays[k]), f"{name} step 2 {k}"
            sw.step3()
            assert all(_same(g, w) for g, w in zip(_results(sw), want)), f"{name} step-wise"
            assert not poisoned(sw.array("c_vals")).any(), f"{name} step-wise"
            for _ in range(3):
                ref.spgemm()
                assert all(_same(g, w) for g, w in zip(_results(ref), want)), f"{name} repeat pass"
                assert not poisoned(ref.array("c_vals")).any(), f"{name} repeat pass"
            ctx.set_graph_replay(True)
            try:
                for _ in range(3):
                    ref.spgemm()
                    assert all(_same(g, w) for g, w in zip(_results(ref), want)), f"{name} graph replay"
                    assert not poisoned(ref.array("c_vals")).any(), f"{name} graph replay"
                    for k in ARRAYS:
                        assert _same(ref.array(k), want_arrays[k]), f"{name} graph replay {k}"
            finally:
                ctx.set_graph_replay(False)
            ref.spgemm()                                           # and a plain repeat pass after the replays
            assert all(_same(g, w) for g, w in zip(_results(ref), want)), f"{name} after replay"


def test_numeric_refresh(pkg, oracle, ctx):
    for name in ("rand_300", "banded_500_AAt", "band_1500"):
        rows, cols, I, J, V, tr = case = CASES[name]
        V2src = _vals(np.random.default_rng(31), len(I))
        order = np.argsort(I.astype(np.int64) * cols + J, kind="stable")
        V2 = V2src[order]
        for comp in (False, True):
            A, B = _tilings(pkg, ctx, case)
            M = pkg.Tiled.from_coo(ctx, rows, B.cols, I, J, np.ones(len(I)))      # (all three are square)
            plan = pkg.CPlan(ctx, A, B, mask=M, complement=comp)
            plan.spgemm()
            A.set_values(V2, "row")
            if tr:
                B.set_values(V2, "col")
            M.set_values(np.full(M.nnz, 7.0))                      # the mask's values do nothing
            plan.step3()
            A2, B2 = _tilings(pkg, ctx, case, V=V2src)
            fresh = pkg.CPlan(ctx, A2, B2, mask=M, complement=comp)
            fresh.spgemm()
            assert all(_same(g, w) for g, w in zip(_results(plan), _results(fresh))), f"{name} {comp}"


def test_row_ranges_concatenate(pkg, oracle, ctx):
    for name in ("powerlaw_600", "banded_500_AAt", "hub_row_4000"):
        rows, cols, I, J, V, tr = case = CASES[name]
        A, B = _tilings(pkg, ctx, case)
        rng = np.random.default_rng(4)
        key = np.unique(rng.integers(0, rows * B.cols, rows * 8, dtype=np.int64))
        MI, MJ = (key // B.cols).astype(np.int32), (key % B.cols).astype(np.int32)
        M = pkg.Tiled.from_coo(ctx, rows, B.cols, MI, MJ, np.ones(len(MI)))
        for comp in (False, True):
            whole = pkg.CPlan(ctx, A, B, mask=M, complement=comp)
            whole.spgemm()
            wrp, wci, wv = whole.export_csr()
            tr_n = A.tile_rows
            for cuts in ([0, tr_n // 2, tr_n], [0, tr_n // 3, 2 * tr_n // 3, tr_n]):
                rps, cis, vs = [np.zeros(1, np.int64)], [], []
                for lo, hi in zip(cuts[:-1], cuts[1:]):
                    p = pkg.CPlan(ctx, A, B, lo, hi, mask=M, complement=comp)
                    p.spgemm()
                    rp, ci, v = p.export_csr()
                    rps.append(rp[1:].astype(np.int64) + rps[-1][-1])
                    cis.append(ci)
                    vs.append(v)
                assert _same(np.concatenate(rps).astype(np.int32), wrp) and _same(np.concatenate(cis), wci) and _same(np.concatenate(vs), wv), \
                    f"{name} {cuts} {comp}"


def test_errors(pkg, ctx):
    rows, cols, I, J, V, tr = CASES["rect_70x40_AAt"]
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    At = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, True)
    wrong = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)           # 70 x 40, but C = A*A^T is 70 x 70
    with pytest.raises(pkg.PemError) as e:
        pkg.CPlan(ctx, A, At, mask=wrong)
    assert e.value.status == PEM_E_INVALID and "70 x 40" in str(e.value)
    d = np.arange(rows, dtype=np.int32)
    good = pkg.Tiled.from_coo(ctx, rows, rows, d, d, np.ones(rows))
    h = C.c_void_p()
    L = pkg.lib()
    assert L.pem_cplan_create_masked(ctx._h, A._h, At._h, good._h, 2, 0, -1, C.byref(h)) == PEM_E_INVALID
    assert b"flags" in L.pem_last_error()
    assert L.pem_cplan_create_masked(ctx._h, A._h, At._h, None, 0, 0, -1, C.byref(h)) == PEM_E_INVALID
    assert b"null" in L.pem_last_error()
    assert not h.value
    plan = pkg.CPlan(ctx, A, At, mask=good)
    for k, v in (("step1_global_sort", 1), ("wide", 0)):
        with pytest.raises(pkg.PemError) as e:
            plan.set_option(k, v)
        assert e.value.status == PEM_E_INVALID
    plan.set_option("step1_global_sort", 0)
    plan.set_option("wide", 1)
    plan.spgemm()
    unmasked = pkg.CPlan(ctx, A, At)
    with pytest.raises(pkg.PemError):
        unmasked.array("c_mtile")                                  # not a masked plan


def test_triangle_count(pkg, ctx):
    rng = np.random.default_rng(11)
    n = 400
    D = np.triu(rng.random((n, n)) < 0.03, 1)
    D = D | D.T
    I, J = np.nonzero(D)
    A = pkg.Tiled.from_coo(ctx, n, n, I.astype(np.int32), J.astype(np.int32), np.ones(len(I)))
    plan = pkg.CPlan(ctx, A, A, mask=A)
    plan.spgemm()
    _, _, v = plan.export_csr()
    Ad = D.astype(np.float64)
    assert v.sum() / 6 == np.trace(Ad @ Ad @ Ad) / 6 and v.sum() > 0


def test_full_size_webbase(pkg, standins, ctx):
    rows, cols, I, J, V = standins.make("webbase-1M", 1.0)
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    full = pkg.CPlan(ctx, A, A)
    full.spgemm()
    c_full = full.export_csr()
    for comp in (False, True):
        plan = pkg.CPlan(ctx, A, A, mask=A, complement=comp)
        plan.spgemm()
        want = maskref.filter_csr(*c_full, I, J, cols, comp)
        got = plan.export_csr()
        assert all(_same(g, w) for g, w in zip(got, want)), f"complement={comp}"
        plan.spgemm()
        assert all(_same(g, w) for g, w in zip(plan.export_csr(), want)), f"complement={comp}: repeat pass"
