"""GPU: step 3's two-pair blocks (later pairs two at a time, a second product gathered beside the first) against the oracle, bit for bit.

One layout (tests/s3blocks.py; test_s3_blocks_cpu.py shows what it reaches) runs in every shallow form of the kernel, in fp64
and fp32, under plus-times, plus-pair (no values) and min-plus, pruned and with prune = 0.  C is poisoned before every step 3 and
must equal the oracle's on the first pass, a warm pass, a graph replay and a step 3 after new operand values; and the kernels
keep the names of their form.
"""
import numpy as np
import pytest
import torch

import s3blocks
import s3cases
from matgen import _vals
from test_gpu_s3_paths import Ref, _device, _kernels_of, _plan, check

pytestmark = pytest.mark.gpu

torch.cuda.is_available()   # (torch's runtime first, as in test_gpu_values.py)

DTYPES = (np.float64, np.float32)
SEMIRINGS = ("plus_times", "plus_pair", "min_plus")
_REFS = {}


def _ref(oracle, case, dtype):
    """C of the layout per semiring, computed once per value type: the options do not change C"""
    key = np.dtype(dtype)
    if key not in _REFS:
        _REFS[key] = Ref(oracle, case, dtype)
    return _REFS[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("name", sorted(s3blocks.FORMS))
def test_blocks_case(pkg, oracle, ctx, name, dtype):
    case = s3blocks.case(name)
    vt = "double" if dtype == np.float64 else "float"
    A, B, M = _device(pkg, ctx, case, dtype)
    ref = _ref(oracle, case, dtype)
    inputs = s3cases.plan_arrays(oracle, case)
    npairs, ntc = int(inputs["pairs_offset"][-1]), len(inputs["pairs_offset"]) - 1
    assert npairs < 2 * ntc
    assert s3cases.form_of(npairs, ntc, case["opts"], "plus_times") == s3blocks.FORMS[name][1]
    plan = _plan(pkg, ctx, case, A, B, M)
    assert plan.get_option("s3_poison") == 1 and plan.get_option("s3_batch") == 0
    for s in SEMIRINGS:
        want = ref(s)
        plan.set_semiring(s)
        ks = _kernels_of(ctx, plan.spgemm if s == "plus_times" else plan.step3)
        if s == "plus_times":                            # the model's inputs are the device's
            for k in ("pairs_offset", "c_tile_nnz_ptr"):
                assert np.array_equal(plan.array(k), inputs[k]), f"{name}: {k}"
        form = s3cases.form_of(npairs, ntc, case["opts"], s)
        assert ks == s3cases.kernel_names(form, vt, s), (name, s, ks)
        check(plan.export_csr(), want, f"{name} {s}")
        plan.spgemm()                                    # a warm pass: C poisoned again
        check(plan.export_csr(), want, f"{name} {s} warm")
    ctx.set_graph_replay(True)
    try:
        for s in ("plus_times", "plus_pair"):
            plan.set_semiring(s)
            for rep in range(3):                         # (the first pass after a change captures, the others replay)
                plan.spgemm()
                check(plan.export_csr(), ref(s), f"{name} {s} replay {rep}")
    finally:
        ctx.set_graph_replay(False)
    # new values for A, step 3 alone
    rows, cols, I, J, _ = s3cases.operands(case)[0]["A"]
    V2 = _vals(np.random.default_rng(77), len(I)).astype(dtype)
    A.set_values(V2[np.lexsort((J, I))], "row")
    plan.set_semiring("plus_times")
    plan.step3()
    check(plan.export_csr(), Ref(oracle, case, dtype, V2)("plus_times"), f"{name} refreshed")
