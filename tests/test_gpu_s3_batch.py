"""GPU: step 3's batched record fetch (PEM_OPT_S3_BATCH) against the serial loop and the oracle, bit for bit.

One layout (tests/s3batch.py) holds every edge of the batching -- batches partly and wholly filled, a second and a third batch,
trips where only some lanes have a later pair, the staging limit on both sides, a partial trip, a tile split across trips and
waves, later pairs that meet nowhere and later pairs with two products -- and runs in every shallow form of the kernel, in fp64
and fp32, under plus-times, plus-pair (no values) and min-plus.  With the option on and off C must equal the oracle's (so the
two equal each other) with C poisoned before every step 3: on the first pass, a warm pass, a graph replay and a step 3 after
new operand values; and the kernels keep the names of their form.
"""
import numpy as np
import pytest
import torch

import s3batch
import s3cases
from matgen import _vals
from test_gpu_s3_paths import Ref, _bits, _device, _kernels_of, _plan, check

pytestmark = pytest.mark.gpu

torch.cuda.is_available()   # (torch's runtime first, as in test_gpu_values.py)

DTYPES = (np.float64, np.float32)
SEMIRINGS = ("plus_times", "plus_pair", "min_plus")
_REFS = {}


def _ref(oracle, case, dtype):
    """C of the layout per semiring, computed once per (mask, value type): the options do not change C"""
    key = (case["mask"], np.dtype(dtype))
    if key not in _REFS:
        _REFS[key] = Ref(oracle, case, dtype)
    return _REFS[key]


def test_layout_reaches_the_edges(oracle):
    """host only: the plan arrays of the layout put the kernel's trips where the batching can go wrong"""
    arr = s3cases.plan_arrays(oracle, s3batch.case("decode_idx32_mark"))
    po, off = arr["pairs_offset"], arr["c_tile_nnz_ptr"]
    assert po[-1] < 2 * (len(po) - 1), "the layout must be shallow"
    tr = s3batch.trips(po, off)
    staged = [t for t in tr if t["staged"]]
    deepest = {int(t["n_of"].max()) for t in staged}
    assert {3, 4, 5, 6, 8, 9} <= deepest, deepest                              # batch edges: 1-3 rounds, a second batch, a third
    assert any({1, 2, 5, 9} <= set(t["n_of"].tolist()) for t in staged)         # mixed trip
    assert any(t["Pn"] == 64 and t["staged"] and 5 in t["n_of"] and t["nvalid"] == 64 for t in tr)
    assert any(t["Pn"] == 65 and not t["staged"] and 5 in t["n_of"] for t in tr)
    assert any(t["nvalid"] < 64 and t["staged"] and t["n_of"][-1] == 5 for t in tr)   # partial trip ending in a 5-pair tile
    ent, npt = np.diff(off), np.diff(po)
    split = [u for u in np.nonzero((ent == 256) & (npt == 5))[0] if off[u] // 256 != (off[u + 1] - 1) // 256]
    assert split, "no 256-entry 5-pair tile across two waves"
    assert sum(1 for t in staged if split[0] in t["tile"]) >= 4                 # ... and across trips: the strip is reused
    m = s3cases.model(po, off, (), "plus_times", False, arr["c_mask"])
    assert {"sh_staged_pn64", "sh_unstaged_pn65", "tile_split_across_waves", "tile_split_across_trips", "trip_partial"} <= m["paths"]
    none, multi = s3batch.later_pair_products(s3batch.tiles())
    assert none > 0 and multi > 0, (none, multi)                                # later pairs that meet nowhere / with two products
    # prune = 0 keeps the dead pairs: batches with dead pairs behind live ones, still shallow
    un = s3cases.plan_arrays(oracle, s3batch.case("unpruned"))
    upo = un["pairs_offset"]
    assert upo[-1] > po[-1] and upo[-1] < 2 * (len(upo) - 1)
    assert any(t["staged"] and int(t["n_of"].max()) >= 6 for t in s3batch.trips(upo, un["c_tile_nnz_ptr"])[-8:])
    # the complement mask empties tiles inside staged trips
    cm = s3cases.plan_arrays(oracle, s3batch.case("complement"))
    mm = s3cases.model(cm["pairs_offset"], cm["c_tile_nnz_ptr"], (), "plus_times", True, cm["c_mask"])
    assert {"empty_tile_inside_trip", "sh_staged"} <= mm["paths"]
    assert cm["pairs_offset"][-1] < 2 * (len(cm["pairs_offset"]) - 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("name", sorted(s3batch.FORMS))
def test_batch_case(pkg, oracle, ctx, name, dtype):
    case = s3batch.case(name)
    masked = case["mask"] is not None
    vt = "double" if dtype == np.float64 else "float"
    A, B, M = _device(pkg, ctx, case, dtype)
    ref = _ref(oracle, case, dtype)
    inputs = s3cases.plan_arrays(oracle, case)
    npairs, ntc = int(inputs["pairs_offset"][-1]), len(inputs["pairs_offset"]) - 1
    assert npairs < 2 * ntc
    assert s3cases.form_of(npairs, ntc, case["opts"], "plus_times", masked) == s3batch.FORMS[name][2]
    plans = {}
    for batch in (1, 0):
        plans[batch] = _plan(pkg, ctx, case, A, B, M)
        assert plans[batch].get_option("s3_batch") == 0                         # the default
        plans[batch].set_option("s3_batch", batch)
        assert plans[batch].get_option("s3_batch") == batch and plans[batch].get_option("s3_poison") == 1
    for s in SEMIRINGS:
        want = ref(s)
        got = {}
        for batch, plan in plans.items():
            plan.set_semiring(s)
            ks = _kernels_of(ctx, plan.spgemm if s == "plus_times" else plan.step3)
            if s == "plus_times":                        # the model's inputs are the device's
                for k in ("pairs_offset", "c_tile_nnz_ptr"):
                    assert np.array_equal(plan.array(k), inputs[k]), f"{name}: {k}"
            form = s3cases.form_of(npairs, ntc, case["opts"], s, masked)
            assert ks == s3cases.kernel_names(form, vt, s), (name, s, batch, ks)
            got[batch] = plan.export_csr()
            check(got[batch], want, f"{name} {s} batch={batch}")
            plan.spgemm()                                # a warm pass: C poisoned again
            check(plan.export_csr(), want, f"{name} {s} batch={batch} warm")
        assert np.array_equal(_bits(got[1][2]), _bits(got[0][2])), f"{name} {s}: batched and serial differ"
    ctx.set_graph_replay(True)
    try:
        for s in ("plus_times", "plus_pair"):
            for batch, plan in plans.items():
                plan.set_semiring(s)
                for rep in range(3):                     # (the first pass after a change captures, the others replay)
                    plan.spgemm()
                    check(plan.export_csr(), ref(s), f"{name} {s} batch={batch} replay {rep}")
    finally:
        ctx.set_graph_replay(False)
    # new values for A, step 3 alone
    rows, cols, I, J, _ = s3cases.operands(case)[0]["A"]
    V2 = _vals(np.random.default_rng(77), len(I)).astype(dtype)
    A.set_values(V2[np.lexsort((J, I))], "row")
    want = Ref(oracle, case, dtype, V2)("plus_times")
    for batch, plan in plans.items():
        plan.set_semiring("plus_times")
        plan.step3()
        check(plan.export_csr(), want, f"{name} refreshed batch={batch}")


def test_option_restarts_the_plan(pkg, oracle, ctx):
    """setting s3_batch takes the plan back to step 2's result, like the other step-3 options: step 3 alone recomputes C"""
    case = s3batch.case("decode_idx32_mark")
    A, B, M = _device(pkg, ctx, case, np.float64)
    plan = _plan(pkg, ctx, case, A, B, M)
    plan.spgemm()
    want = _ref(oracle, case, np.float64)("plus_times")
    for batch in (1, 0):                                 # (each differs from the value before it: setting the same value changes nothing)
        plan.set_option("s3_batch", batch)
        with pytest.raises(pkg.PemError):
            plan.export_csr()                            # C is stale until step 3 has run again
        plan.step3()
        check(plan.export_csr(), want, f"batch={batch}")
