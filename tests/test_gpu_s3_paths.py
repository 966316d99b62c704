"""GPU: every step-3 kernel path of tests/s3cases.py, bit for bit, with C poisoned before each step 3.

Each case's layout is built for the paths it claims (test_s3_cover_cpu.py shows the model reaches them).  Here the device plan
must hold the model's inputs (pairs_offset, c_tile_nnz_ptr), run the kernels of the model's form, and give C bit for bit:
plus-times against the oracle's serial chain (its float chain for fp32), the other semirings against tests/semiringref.py.
Every plan runs with PEM_OPT_S3_POISON = 1, so an entry step 3 leaves unwritten keeps a NaN pattern no kernel computes, on the
first pass, a warm pass, a graph replay and a step 3 after new operand values alike.
"""
import numpy as np
import pytest
import torch

import maskref
import s3cases
import semiringref as sr
from matgen import _vals
from s3cases import poisoned

pytestmark = pytest.mark.gpu

torch.cuda.is_available()   # (torch's runtime first, as in test_gpu_values.py)

CASES = s3cases.cases()
DTYPES = (np.float64, np.float32)


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def check(got, want, label):
    rp, ci, v = got
    wrp, wci, wv = want
    assert np.array_equal(rp, wrp) and np.array_equal(ci, wci), f"{label}: structure"
    assert not poisoned(v).any(), f"{label}: {int(poisoned(v).sum())} of {len(v)} entries were not written by step 3"
    assert v.dtype == wv.dtype and np.array_equal(_bits(v), _bits(wv)), \
        f"{label}: {int((_bits(v) != _bits(wv)).sum())} of {len(v)} values differ"


def _kernels_of(ctx, run):
    """names of the step-3 kernels one call runs (as test_gpu_semiring.py)"""
    ctx.set_kernel_profiling(True)
    ctx.reset_kernel_stats()
    try:
        run()
        ctx.synchronize()
        return sorted(k for k in ctx.kernel_stats() if k.startswith("s3_"))
    finally:
        ctx.set_kernel_profiling(False)


def _cast(coo, dtype):
    return coo[:4] + (np.asarray(coo[4]).astype(dtype),)


class Ref:
    """C of a case under each semiring, in the value type, restricted as the plan restricts it (tile rows, mask)"""

    def __init__(self, oracle, case, dtype, A_vals=None):
        self.oracle, self.case, self.dtype = oracle, case, dtype
        self.ops, self.mask = s3cases.operands(case)
        A = self.ops["A"] if A_vals is None else self.ops["A"][:4] + (A_vals,)
        self.A, self.B = _cast(A, dtype), _cast(self.ops["B"], dtype)
        self.cache = {}

    def _restrict(self, rp, ci, v):
        ncols = self.B[1]
        if self.mask is not None:
            rp, ci, v = maskref.filter_csr(rp, ci, v, self.mask[0], self.mask[1], ncols, complement=True)
        if self.case["tile_rows"]:
            lo, hi = self.case["tile_rows"]
            r0, r1 = 16 * lo, min(16 * hi, self.A[0])
            rp, ci, v = rp[r0:r1 + 1] - rp[r0], ci[rp[r0]:rp[r1]], v[rp[r0]:rp[r1]]
        return np.asarray(rp, np.int32), np.asarray(ci, np.int32), v

    def __call__(self, semiring):
        if semiring not in self.cache:
            if semiring == "plus_times":
                f32 = self.dtype == np.float32
                wide = lambda c: c[:4] + (c[4].astype(np.float64),)   # noqa: E731  (float values widened exactly)
                o = self.oracle
                rp, ci, v = o.csr_spgemm(o.Csr(*wide(self.A)), o.Csr(*wide(self.B)), f32=f32).arrays()
                v = v.astype(self.dtype)
            else:
                rp, ci, v = sr.spgemm(sr.coo_to_csr(*self.A), sr.coo_to_csr(*self.B), self.B[1], semiring, self.dtype)
            self.cache[semiring] = self._restrict(rp, ci, v)
        return self.cache[semiring]


def _device(pkg, ctx, case, dtype):
    ops, mask = s3cases.operands(case)
    A = pkg.Tiled.from_coo(ctx, *_cast(ops["A"], dtype), dtype=dtype)
    B = pkg.Tiled.from_coo(ctx, *_cast(ops["B"], dtype), dtype=dtype)
    M = None
    if mask is not None:
        n = 16 * ops["T"]
        M = pkg.Tiled.from_coo(ctx, n, n, mask[0], mask[1], np.ones(len(mask[0])))
    return A, B, M


def _plan(pkg, ctx, case, A, B, M, poison=1):
    lo, hi = case["tile_rows"] or (0, -1)
    plan = pkg.CPlan(ctx, A, B, lo, hi, mask=M, complement=M is not None)
    for k, v in case["opts"]:
        plan.set_option(k, v)
    plan.set_option("s3_poison", poison)
    return plan


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_path_case(pkg, oracle, ctx, name, dtype):
    case = CASES[name]
    vt = "double" if dtype == np.float64 else "float"
    A, B, M = _device(pkg, ctx, case, dtype)
    ref = Ref(oracle, case, dtype)
    inputs = s3cases.plan_arrays(oracle, case)
    plan = _plan(pkg, ctx, case, A, B, M)
    assert plan.get_option("s3_poison") == 1
    for s in sr.SEMIRINGS:
        plan.set_semiring(s)
        ks = _kernels_of(ctx, plan.spgemm if s == "plus_times" else plan.step3)
        if s == "plus_times":                            # the model's inputs are the device's
            for k in ("pairs_offset", "c_tile_nnz_ptr"):
                assert np.array_equal(plan.array(k), inputs[k]), f"{name}: {k}"
        m = s3cases.model(inputs["pairs_offset"], inputs["c_tile_nnz_ptr"], case["opts"], s, M is not None, inputs["c_mask"])
        assert ks == s3cases.kernel_names(m["form"], vt, s), (name, s, m["form"], ks)
        check(plan.export_csr(), ref(s), f"{name} {s}")
        plan.spgemm()                                    # a warm pass: C poisoned again, step 3 must write it all again
        check(plan.export_csr(), ref(s), f"{name} {s} warm")
    ctx.set_graph_replay(True)
    try:
        for s in ("plus_times", "max_times", "plus_pair"):
            plan.set_semiring(s)
            for rep in range(3):                         # (the first pass after a change captures, the others replay)
                plan.spgemm()
                check(plan.export_csr(), ref(s), f"{name} {s} replay {rep}")
    finally:
        ctx.set_graph_replay(False)
    # new values for A, step 3 alone
    plan.set_semiring("plus_times")
    rows, cols, I, J, _ = s3cases.operands(case)[0]["A"]
    V2 = _vals(np.random.default_rng(77), len(I)).astype(dtype)
    order = np.lexsort((J, I))
    A.set_values(V2[order], "row")
    plan.step3()
    check(plan.export_csr(), Ref(oracle, case, dtype, V2)("plus_times"), f"{name} refreshed")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
def test_poison_alone_is_caught(pkg, oracle, ctx, dtype):
    """s3_poison = 2 fills C and runs no step-3 kernel: every value holds the fill, and check() rejects the output"""
    for name in ("shallow", "deep_band"):
        case = CASES[name]
        A, B, M = _device(pkg, ctx, case, dtype)
        plan = _plan(pkg, ctx, case, A, B, M)
        plan.spgemm()
        check(plan.export_csr(), Ref(oracle, case, dtype)("plus_times"), name)   # (1: correct values over the fill)
        plan.set_option("s3_poison", 2)
        assert _kernels_of(ctx, plan.spgemm) == []
        got = plan.export_csr()
        assert poisoned(got[2]).all() and poisoned(plan.array("c_vals")).all()
        with pytest.raises(AssertionError, match="not written"):
            check(got, Ref(oracle, case, dtype)("plus_times"), name)
        plan.set_option("s3_poison", 0)                  # off: the default kernels, the same C
        plan.spgemm()
        check(plan.export_csr(), Ref(oracle, case, dtype)("plus_times"), f"{name} poison off")
