"""GPU: semirings of step 3 (pem_cplan_set_semiring, CPlan(..., semiring=...)).

Every plan is held to: C's structure (rowptr, colidx) equals the plus-times plan's; min/max values equal the numpy statement
(tests/semiringref.py) exactly, with -0 == +0; plus_pair and lor_land are exact; and plus-times after a round trip through the
other semirings is bit-identical to a fresh plan.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import semiringref as sr
from matgen import _vals, cases
from s3cases import poisoned

pytestmark = pytest.mark.gpu

torch.cuda.is_available()   # (torch's runtime first, as in test_gpu_values.py)

CASES = cases()
PEM_E_INVALID, PEM_E_STATE = -1, -6
DTYPES = (np.float64, np.float32)


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _operands(case, V=None):
    """CSR triples of A and B as the plan multiplies them"""
    rows, cols, I, J, V0, tr = case
    V = V0 if V is None else V
    A = sr.coo_to_csr(rows, cols, I, J, V)
    B = sr.transpose_csr(rows, cols, *A) if tr else A
    return A, B, (rows if tr else cols)


def _tilings(pkg, ctx, case, dtype=np.float64, V=None):
    rows, cols, I, J, V0, tr = case
    V = V0 if V is None else V
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=dtype)
    B = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, True, dtype=dtype) if tr else A
    return A, B


def _check(got, want, label):
    rp, ci, v = got
    wrp, wci, wv = want
    assert np.array_equal(rp, wrp) and np.array_equal(ci, wci), f"{label}: structure"
    assert v.dtype == wv.dtype and sr.same_values(v, wv), f"{label}: values"


def _expected(ref_ops, semiring, dtype, cache):
    key = (semiring, np.dtype(dtype).name)
    if key not in cache:
        A, B, nc = ref_ops
        cache[key] = sr.spgemm(A, B, nc, semiring, dtype)
    return cache[key]


def _kernels_of(ctx, plan, run):
    """names of the step-3 kernels one call runs"""
    ctx.set_kernel_profiling(True)
    ctx.reset_kernel_stats()
    try:
        run()
        ctx.synchronize()
        return sorted(k for k in ctx.kernel_stats() if k.startswith("s3_"))
    finally:
        ctx.set_kernel_profiling(False)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case_every_semiring(pkg, ctx, name, dtype):
    case = CASES[name]
    A, B = _tilings(pkg, ctx, case, dtype)
    ref_ops, cache = _operands(case), {}
    base = pkg.CPlan(ctx, A, B)
    base.spgemm()
    brp, bci, bv = base.export_csr()
    plan = pkg.CPlan(ctx, A, B)
    plan.spgemm()                                          # one symbolic pass, then step 3 per semiring
    for s in sr.NEW:
        plan.set_semiring(s)
        assert plan.semiring == s
        plan.step3()
        got = plan.export_csr()
        assert np.array_equal(got[0], brp) and np.array_equal(got[1], bci), f"{name} {s}: structure differs from plus-times"
        _check(got, _expected(ref_ops, s, dtype, cache), f"{name} {s}")
        if s == "min_plus":                                # and the same through a pem_spgemm pass on a fresh plan
            fresh = pkg.CPlan(ctx, A, B, semiring=s)
            fresh.spgemm()
            assert all(_same_bits(g, w) for g, w in zip(fresh.export_csr(), got)), f"{name} {s}: fresh plan"
            fresh.close()
    plan.set_semiring("plus_times")
    plan.step3()
    assert all(_same_bits(g, w) for g, w in zip(plan.export_csr(), (brp, bci, bv))), f"{name}: plus-times after the round trip"
    assert _same_bits(plan.array("c_vals"), base.array("c_vals"))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("semiring", sr.NEW)
def test_special_values(pkg, ctx, semiring, dtype):
    """NaN, +-inf and -0.0 in A and B; under plus_pair every value NaN, the counts unchanged"""
    rng = np.random.default_rng(21)
    specials = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.5, -2.0, 0.75])
    for name in ("rand_300", "band_1500", "dense_48", "banded_500_AAt"):
        rows, cols, I, J, V, tr = CASES[name]
        V2 = np.where(rng.random(len(V)) < 0.4, rng.choice(specials, len(V)), V)
        if semiring == "plus_pair":
            V2 = np.full(len(V), np.nan)
        case = (rows, cols, I, J, V2, tr)
        A, B = _tilings(pkg, ctx, case, dtype)
        plan = pkg.CPlan(ctx, A, B, semiring=semiring)
        plan.spgemm()
        with np.errstate(all="ignore"):
            want = sr.spgemm(*_operands(case), semiring, dtype)
        _check(plan.export_csr(), want, f"{name} {semiring}")
        if semiring == "plus_pair":                       # the counts of the original values
            A0, B0 = _tilings(pkg, ctx, CASES[name], dtype)
            p0 = pkg.CPlan(ctx, A0, B0, semiring="plus_pair")
            p0.spgemm()
            assert _same_bits(p0.export_csr()[2], plan.export_csr()[2]), name


# option sets that reach every dispatch branch of step 3; the form each one takes follows from the plan's shape (_form), and
# test_dispatch_covers_every_form checks that together they reach all five
BRANCHES = [
    ("diag_100", ()),                                       # shallow: the decode form (64-bit, shuffle search)
    ("diag_100", (("s3_decode", 0),)),                      # shallow without decode: Ctiles_rowColIdx, entry per lane
    ("powerlaw_600", ()),
    ("powerlaw_600", (("s3_epw", 2), ("s3_mark", 0))),
    ("rand_300", (("wide", 0),)),                           # 16 lanes per tile
    ("rand_300", (("step1_global_sort", 1),)),              # the global-sort step 1 takes the 16-lanes-per-tile step 3 too
    ("dense_48", ()),                                       # deep
    ("band_1500", ()),                                      # deep + the band pair with many-pair tiles
    ("band_1500", (("s3_band", 0),)),                       # deep without the band kernel
    ("banded_500_AAt", (("s3_idx64", 1),)),
    ("blockrows_1600", (("prune", 0),)),
]
FORMS = ("decode", "wide", "base", "deep", "deep,band")


def _form(plan, options):
    """the step-3 form pem_spgemm takes on this plan (step3.hip, s3_launch)"""
    o = dict(options)
    if o.get("wide", 1) == 0 or o.get("step1_global_sort", 0) == 1:
        return "base"
    i = plan.info()
    if i["npairs"] >= 2 * i["ntiles_c"]:
        return "deep,band" if o.get("s3_band", 1) else "deep"
    return "decode" if o.get("s3_decode", 1) else "wide"


def _names(form, vt, semiring):
    return {"decode": [f"s3_accumulate_wide_kernel<{vt},decode,{semiring}>"], "wide": [f"s3_accumulate_wide_kernel<{vt},{semiring}>"],
            "base": [f"s3_accumulate_kernel<{vt},{semiring}>"], "deep": [f"s3_accumulate_wide_kernel<{vt},deep,{semiring}>"],
            "deep,band": sorted([f"s3_accumulate_wide_kernel<{vt},deep,band,{semiring}>", f"s3_band_kernel<{vt},{semiring}>"])}[form]


@pytest.mark.parametrize("semiring", sr.NEW)
@pytest.mark.parametrize("name,options", BRANCHES, ids=lambda x: x if isinstance(x, str) else ("-".join(f"{k}{v}" for k, v in x) or "default"))
def test_dispatch_branches(pkg, ctx, name, options, semiring):
    case = CASES[name]
    for dtype in DTYPES:
        A, B = _tilings(pkg, ctx, case, dtype)
        plan = pkg.CPlan(ctx, A, B, semiring=semiring)
        for k, v in options:
            plan.set_option(k, v)
        ks = _kernels_of(ctx, plan, plan.spgemm)
        form = _form(plan, options)
        assert ks == _names(form, "double" if dtype == np.float64 else "float", semiring), (form, ks)
        want = sr.spgemm(*_operands(case), semiring, dtype)
        _check(plan.export_csr(), want, f"{name} {options} {semiring} {dtype.__name__}")
        plan.spgemm()                                              # repeat pass on the same options
        _check(plan.export_csr(), want, f"{name} {options} {semiring} repeat")


def test_dispatch_covers_every_form(pkg, ctx):
    forms = set()
    for name, options in BRANCHES:
        A, B = _tilings(pkg, ctx, CASES[name])
        plan = pkg.CPlan(ctx, A, B)
        for k, v in options:
            plan.set_option(k, v)
        plan.spgemm()
        forms.add(_form(plan, options))
    assert forms == set(FORMS), forms


def test_plus_times_kernel_names_unchanged(pkg, ctx):
    A, B = _tilings(pkg, ctx, CASES["band_1500"])
    plan = pkg.CPlan(ctx, A, B)
    assert _kernels_of(ctx, plan, plan.spgemm) == ["s3_accumulate_wide_kernel<double,deep,band>", "s3_band_kernel<double>"]
    A, B = _tilings(pkg, ctx, CASES["diag_100"], np.float32)
    plan = pkg.CPlan(ctx, A, B)
    assert _kernels_of(ctx, plan, plan.spgemm) == ["s3_accumulate_wide_kernel<float,decode,idx32,mark>"]


def test_band_pair_reaches_many_pair_tiles(pkg, ctx):
    """band_1500 holds C tiles of 8+ pairs, which only s3_band_kernel computes: their values must be right under every semiring"""
    case = CASES["band_1500"]
    A, B = _tilings(pkg, ctx, case)
    plan = pkg.CPlan(ctx, A, B)
    plan.spgemm()
    po = plan.array("pairs_offset")
    assert (np.diff(po) >= 8).sum() > 0
    for s in sr.NEW:
        plan.set_semiring(s)
        plan.step3()
        _check(plan.export_csr(), sr.spgemm(*_operands(case), s), s)


@pytest.mark.parametrize("semiring", sr.NEW)
def test_masked_and_complement(pkg, ctx, semiring):
    for name in ("rand_300", "band_1500", "banded_500_AAt", "powerlaw_600"):
        case = CASES[name]
        rows, cols, I, J, V, tr = case
        A, B = _tilings(pkg, ctx, case)
        nc = B.cols
        rng = np.random.default_rng(6)
        key = np.unique(rng.integers(0, rows * nc, rows * 6, dtype=np.int64))
        MI, MJ = (key // nc).astype(np.int32), (key % nc).astype(np.int32)
        M = pkg.Tiled.from_coo(ctx, rows, nc, MI, MJ, np.ones(len(MI)))
        full = sr.spgemm(*_operands(case), semiring)
        for comp in (False, True):
            base = pkg.CPlan(ctx, A, B, mask=M, complement=comp)
            base.spgemm()
            brp, bci, bv = base.export_csr()
            plan = pkg.CPlan(ctx, A, B, mask=M, complement=comp, semiring=semiring)
            plan.spgemm()
            got = plan.export_csr()
            assert np.array_equal(got[0], brp) and np.array_equal(got[1], bci), f"{name} {comp}: structure"
            _check(got, sr.filter_csr(*full, nc, MI, MJ, comp), f"{name} complement={comp}")
            plan.set_semiring("plus_times")
            plan.step3()
            assert _same_bits(plan.export_csr()[2], bv)


@pytest.mark.parametrize("semiring", ["min_plus", "plus_pair", "max_times"])
def test_row_ranges_concatenate(pkg, ctx, semiring):
    for name in ("powerlaw_600", "banded_500_AAt", "band_1500"):
        case = CASES[name]
        A, B = _tilings(pkg, ctx, case)
        want = sr.spgemm(*_operands(case), semiring)
        tr_n = A.tile_rows
        for cuts in ([0, tr_n // 2, tr_n], [0, tr_n // 3, 2 * tr_n // 3, tr_n]):
            rps, cis, vs = [np.zeros(1, np.int64)], [], []
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                p = pkg.CPlan(ctx, A, B, lo, hi, semiring=semiring)
                p.spgemm()
                rp, ci, v = p.export_csr()
                rps.append(rp[1:].astype(np.int64) + rps[-1][-1])
                cis.append(ci)
                vs.append(v)
            _check((np.concatenate(rps), np.concatenate(cis), np.concatenate(vs)), want, f"{name} {cuts}")


def test_stale_rule(pkg, ctx):
    case = CASES["rand_300"]
    A, B = _tilings(pkg, ctx, case)
    plan = pkg.CPlan(ctx, A, B)
    plan.spgemm()
    sym = {k: plan.array(k) for k in ("pairs_a", "pairs_b", "c_mask", "c_tile_nnz_ptr", "c_tile_colidx")}
    plan.set_semiring("plus_times")                                # the current one: nothing goes stale
    plan.export_csr()
    plan.set_semiring("min_plus")
    for call in (plan.export_csr, plan.export_coo, lambda: plan.array("c_vals")):
        with pytest.raises(pkg.PemError) as e:
            call()
        assert e.value.status == PEM_E_STATE and "semiring" in str(e.value)
    d = [torch.empty(n, dtype=t, device="cuda") for n, t in ((301, torch.int32), (plan.info()["nnz_c"], torch.int32), (plan.info()["nnz_c"], torch.float64))]
    with pytest.raises(pkg.PemError) as e:
        plan.export_csr_device(*(x.data_ptr() for x in d))
    assert e.value.status == PEM_E_STATE
    for k, v in sym.items():                                       # the symbolic arrays stay readable
        assert np.array_equal(plan.array(k), v), k
    plan.set_semiring("max_plus")                                  # still stale
    with pytest.raises(pkg.PemError):
        plan.export_csr()
    plan.step3()
    _check(plan.export_csr(), sr.spgemm(*_operands(case), "max_plus"), "after step 3")
    plan.set_semiring("plus_pair")
    with pytest.raises(pkg.PemError):
        plan.export_csr()
    plan.spgemm()                                                  # a whole pass clears it too
    _check(plan.export_csr(), sr.spgemm(*_operands(case), "plus_pair"), "after pem_spgemm")


def test_numeric_refresh_then_new_semiring(pkg, ctx):
    for name in ("rand_300", "banded_500_AAt", "band_1500"):
        rows, cols, I, J, V, tr = case = CASES[name]
        V2src = _vals(np.random.default_rng(41), len(I))
        order = np.argsort(I.astype(np.int64) * cols + J, kind="stable")
        A, B = _tilings(pkg, ctx, case)
        plan = pkg.CPlan(ctx, A, B, semiring="min_plus")
        plan.spgemm()
        A.set_values(V2src[order], "row")
        if tr:
            B.set_values(V2src[order], "col")
        plan.set_semiring("max_times")
        plan.step3()
        _check(plan.export_csr(), sr.spgemm(*_operands(case, V2src), "max_times"), f"{name} refreshed, max_times")
        A.set_values(V[order], "row")                              # back to the old values: the current semiring recomputes
        if tr:
            B.set_values(V[order], "col")
        with pytest.raises(pkg.PemError):
            plan.export_csr()
        plan.step3()
        _check(plan.export_csr(), sr.spgemm(*_operands(case), "max_times"), f"{name} refreshed back")


def test_warm_passes_and_graph_replay(pkg, ctx):
    for name in ("rand_300", "band_1500", "banded_500_AAt"):
        case = CASES[name]
        A, B = _tilings(pkg, ctx, case)
        ref_ops, cache = _operands(case), {}
        base = pkg.CPlan(ctx, A, B)
        base.spgemm()
        want_pt = base.export_csr()
        plan = pkg.CPlan(ctx, A, B, semiring="min_plus")
        plan.set_option("s3_poison", 1)                            # C holds a NaN fill before every step 3, replays included
        for _ in range(3):                                         # warm repeat passes
            plan.spgemm()
            _check(plan.export_csr(), _expected(ref_ops, "min_plus", np.float64, cache), f"{name} warm")
            assert not poisoned(plan.export_csr()[2]).any()
        ctx.set_graph_replay(True)
        try:
            for s in ("min_plus", "plus_pair", "plus_times", "max_plus", "lor_land"):
                plan.set_semiring(s)
                for _ in range(3):                                 # (the first pass after a change captures again)
                    plan.spgemm()
                    got = plan.export_csr()
                    assert not poisoned(got[2]).any(), f"{name} replay {s}"
                    if s == "plus_times":
                        assert all(_same_bits(g, w) for g, w in zip(got, want_pt)), f"{name} replay plus_times"
                    else:
                        _check(got, _expected(ref_ops, s, np.float64, cache), f"{name} replay {s}")
        finally:
            ctx.set_graph_replay(False)
        plan.spgemm()
        _check(plan.export_csr(), _expected(ref_ops, "lor_land", np.float64, cache), f"{name} after replay")
        assert not poisoned(plan.export_csr()[2]).any()


def test_errors(pkg, ctx):
    A, B = _tilings(pkg, ctx, CASES["rand_50"])
    plan = pkg.CPlan(ctx, A, B)
    L = pkg.lib()
    for bad in (-1, 6, 100):
        assert L.pem_cplan_set_semiring(plan._h, bad) == PEM_E_INVALID
        assert b"unknown semiring" in L.pem_last_error()
    assert L.pem_cplan_set_semiring(None, 1) == PEM_E_INVALID
    v = C.c_int(-7)
    assert L.pem_cplan_get_semiring(None, C.byref(v)) == PEM_E_INVALID
    assert L.pem_cplan_get_semiring(plan._h, None) == PEM_E_INVALID
    assert L.pem_cplan_get_semiring(plan._h, C.byref(v)) == 0 and v.value == 0
    assert plan.semiring == "plus_times"
    with pytest.raises(ValueError):
        plan.set_semiring("min_times")
    with pytest.raises(ValueError):
        pkg.CPlan(ctx, A, B, semiring="tropical")
    assert pkg.SEMIRINGS == dict(plus_times=0, min_plus=1, max_plus=2, max_times=3, plus_pair=4, lor_land=5)
    # the semiring is no option: PEM_OPT_WIDE = 0 and the global-sort step 1 combine with every semiring
    plan.set_option("wide", 0)
    plan.set_semiring("lor_land")
    plan.set_option("step1_global_sort", 1)
    plan.spgemm()
    assert plan.semiring == "lor_land"
    _check(plan.export_csr(), sr.spgemm(*_operands(CASES["rand_50"]), "lor_land"), "wide 0")


def test_triangle_count_any_values(pkg, ctx):
    rng = np.random.default_rng(12)
    n = 500
    D = np.triu(rng.random((n, n)) < 0.03, 1)
    D = D | D.T
    I, J = np.nonzero(D)
    V = rng.uniform(-3, 3, len(I))
    V[::7] = 0.0                                                   # values, zeros among them, do not matter
    A = pkg.Tiled.from_coo(ctx, n, n, I.astype(np.int32), J.astype(np.int32), V)
    plan = pkg.CPlan(ctx, A, A, mask=A, semiring="plus_pair")
    plan.spgemm()
    _, _, v = plan.export_csr()
    Ad = D.astype(np.float64)
    tri = np.trace(Ad @ Ad @ Ad) / 6
    assert v.sum() / 6 == tri and tri > 0


def test_min_plus_hops_bellman_ford(pkg, ctx):
    """D_1 = W, D_{k+1} = D_k (x) W under min_plus, each hop tiling the exported C as the next A; W carries a zero-weight diagonal
    (staying put costs nothing), so D_k is the shortest path of at most k edges: CPU Bellman-Ford limited to k rounds"""
    rng = np.random.default_rng(13)
    n = 250
    key = np.unique(rng.integers(0, n * n, 1000, dtype=np.int64))
    I, J = key // n, key % n
    off = I != J
    I, J = np.concatenate([I[off], np.arange(n)]), np.concatenate([J[off], np.arange(n)])
    W = np.where(I == J, 0.0, rng.integers(1, 40, len(I)) * 0.25)
    Wt = pkg.Tiled.from_coo(ctx, n, n, I.astype(np.int32), J.astype(np.int32), W)
    Wd = np.full((n, n), np.inf)
    Wd[I, J] = W
    dist = Wd.copy()                                               # Bellman-Ford from every source: at most 1 edge
    Dt, DI, DJ, DV = Wt, I, J, W
    for hop in range(3):
        plan = pkg.CPlan(ctx, Dt, Wt, semiring="min_plus")
        plan.spgemm()
        rp, ci, v = plan.export_csr()
        dist = np.minimum(dist, np.min(dist[:, :, None] + Wd[None, :, :], axis=1))
        r = np.repeat(np.arange(n), np.diff(rp))
        got = np.full((n, n), np.inf)
        got[r, ci] = v
        assert np.array_equal(got, dist), f"hop {hop + 2}"
        assert np.array_equal(np.isfinite(dist), np.isfinite(got)) and len(ci) == np.isfinite(dist).sum()
        DI, DJ, DV = r.astype(np.int32), ci, v
        Dt = pkg.Tiled.from_coo(ctx, n, n, DI, DJ, DV)             # the exported C is the next hop's A (its pattern grows)


def test_full_size_webbase(pkg, standins, ctx):
    rows, cols, I, J, V = standins.make("webbase-1M", 1.0)
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    ops = sr.coo_to_csr(rows, cols, I, J, V)
    base = pkg.CPlan(ctx, A, A)
    base.spgemm()
    brp, bci, _ = base.export_csr()
    base.close()
    plan = pkg.CPlan(ctx, A, A)
    plan.spgemm()
    for s in ("min_plus", "plus_pair"):
        plan.set_semiring(s)
        plan.step3()
        got = plan.export_csr()
        assert np.array_equal(got[0], brp) and np.array_equal(got[1], bci), s
        want = sr.spgemm(ops, ops, cols, s)
        _check(got, want, s)
        plan.spgemm()                                              # warm pass under the semiring
        _check(plan.export_csr(), want, f"{s} repeat")
        del got, want
