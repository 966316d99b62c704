"""Negative controls of the sequence test: where a deliberate mistake of the MODEL (seqmodel.MUTATIONS) first shows.

first_divergence(program, mutation) runs the true model and the mutated one side by side and returns (step, where) of the first
point at which they differ in something tests/seqrun.py observes -- the status of a call, the handle a step wrote, a dense
result (every array of it; of a solve also the iteration that set the status, which res->launches follows from), or, at an audit,
any live handle (a factor's ilu0_info fields included; of a hierarchy the info fields and every level's A_l, P_l, R_l).  A library that follows the
true model must make the runner report its mismatch exactly there: tests/test_gpu_seq.py runs each NEGATIVE seed under its
mutation and asserts that, tests/test_seq_cpu.py asserts that the committed figures below are what first_divergence gives.  No GPU
import.
"""
import numpy as np

import seqmodel as sm

AUDIT_EVERY = 10     # tests/seqrun.py's

# mutation -> (seed, (step, where)); where is the runner's: "step", "audit" or "after the refusal"
NEGATIVE = {
    "no_bump": (103, (19, "audit")),
    "stale_vals_t": (101, (9, "audit")),
    "no_option_reset": (102, (19, "audit")),
    "concat_stale_block": (1406, (21, "step")),
    "ilu0_stale_source": (1408, (9, "step")),
    "trsv_stale_values": (1401, (8, "step")),
    "amg_stale_weights": (2102, (21, "step")),
    "krylov_stale_factor": (2102, (37, "step")),
    "colour_ties_high": (2101, (15, "step")),
}


def _tiling_differs(a, b, kind="exact", transposed_too=True):
    if (a.rows, a.cols, a.nnz) != (b.rows, b.cols, b.nnz) or not np.array_equal(a.ci, b.ci) or not sm.same(a.vals, b.vals, kind):
        return True
    if transposed_too and a.prov is not None and a.prov[0] == "ilu0" and not np.array_equal(sm.pivot_fields(a), sm.pivot_fields(b)):
        return True                      # (the audit's ilu0_info; its trsv_info reads the pattern alone, which no mutation touches)
    return transposed_too and not sm.same(a.vals_t, b.vals_t)


def _plan_differs(true, mut, a, b):
    if true.current(a) != mut.current(b) or a.options != b.options or a.semiring != b.semiring:
        return True
    if (a.state >= 2) != (b.state >= 2):   # (the audit reads the symbolic arrays from step 2 on)
        return True
    if true.current(a):
        kind = "minmax" if a.c_semiring in sm.MINMAX else "exact"
        return not (np.array_equal(a.C[0], b.C[0]) and np.array_equal(a.C[1], b.C[1]) and sm.same(a.C[2], b.C[2], kind))
    return False


def _hierarchy_differs(true, mut, hid):
    """the audit of a hierarchy: the info fields, and A_l, P_l, R_l of every level"""
    a, b = true.levels(true.h[hid]), mut.levels(mut.h[hid])
    if not np.array_equal(true.amg_fields(true.h[hid]), mut.amg_fields(mut.h[hid])):
        return True
    for L, K in zip(a, b):
        for name in "APR":
            if L[name] is not None and not (np.array_equal(L[name][3], K[name][3]) and sm.same(L[name][4], K[name][4])):
                return True
    return False


def _audit_differs(true, mut, tids, pids, hids=()):
    return any(_tiling_differs(true.t[i], mut.t[i]) for i in tids) or any(_plan_differs(true, mut, true.p[i], mut.p[i]) for i in pids) \
        or any(_hierarchy_differs(true, mut, i) for i in hids)


def first_divergence(prog, mutation):
    true, mut = sm.Model(), sm.Model((mutation,))
    for i, rec in enumerate(prog):
        named_t, named_p = [h for h in rec[1] if h in true.t], [h for h in rec[1] if h in true.p]
        named_h = [h for h in rec[1] if h in true.h]
        r, q = true.apply(rec), mut.apply(rec)
        if r.status != q.status:
            return (i, "step")
        if r.status != 0:
            if _audit_differs(true, mut, named_t, named_p, named_h):
                return (i, "after the refusal")
        else:
            if r.wrote in true.t and _tiling_differs(true.t[r.wrote], mut.t[r.wrote], r.kind, transposed_too=False):
                return (i, "step")
            if r.wrote in true.p:
                a, b = true.p[r.wrote], mut.p[r.wrote]
                if not (np.array_equal(a.C[1], b.C[1]) and sm.same(a.C[2], b.C[2], r.kind)):
                    return (i, "step")
            if r.out is not None:
                x, y = (r.out, q.out) if isinstance(r.out, tuple) else ((r.out,), (q.out,))
                if any(not (sm.same(u, v, r.kind) if np.asarray(u).dtype.kind == "f" else np.array_equal(u, v)) for u, v in zip(x, y)):
                    return (i, "step")
            if r.extra is not None and r.extra["stop_iter"] != q.extra["stop_iter"]:     # (res->launches follows from it)
                return (i, "step")
        if (i + 1) % AUDIT_EVERY == 0 or i + 1 == len(prog):
            if _audit_differs(true, mut, list(true.t), list(true.p), list(true.h)):
                return (i, "audit")
    return None
