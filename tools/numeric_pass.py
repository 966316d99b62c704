"""Numeric-only passes: new values on an existing tiling (pem_tiled_set_values_device), C recomputed by pem_spgemm_step3 alone.

    python tools/numeric_pass.py [--passes 20] [--warmup 3] [--only webbase-1M,...] [--out result.json]

Per workload, on the seeded stand-ins, after warm-ups and over --passes passes (host clock around work that ends in a device
synchronisation; the refresh kernel's time from the library's per-kernel device events, in a loop of its own):
  (a) a warm pem_spgemm pass, graph replay off;
  (b) set_values_device alone: the first call (order maps built) and the steady state;
  (c) set_values_device + pem_spgemm_step3 -- the numeric pass;
and the refresh kernel's achieved bandwidth against the 28 B per fp64 entry its copy needs (V read, vals + vals_t written,
one int32 map read; the kernel also reads the vals_t slot map: 32 B moved).  Before any timing, (c)'s C is checked bit for bit
against a fresh pipeline (conversion, plan, steps 1-3) built on the new values.  mc2depi is A*A^T: both tilings are refreshed
from the same array, A in row-major order and A^T in column-major order.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

WORKLOADS = [("webbase-1M", False), ("webbase-1M-r2", False), ("scircuit", False), ("mc2depi", True), ("cage15", False)]
COMPULSORY_B = {8: 28, 4: 16}    # V + map read, vals + vals_t written, per entry
MOVED_B = {8: 32, 4: 20}         # ... + the vals_t slot map


def _ms(fn, ctx):
    ctx.synchronize()
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _stats(xs):
    return dict(median_ms=statistics.median(xs), mean_ms=statistics.fmean(xs), min_ms=min(xs), n=len(xs))


def run(pkg, standins, torch, name, aat, passes, warmup):
    rows, cols, I, J, V = standins.make(name, 1.0)
    order = np.argsort(I.astype(np.int64) * cols + J, kind="stable")          # source entries in CSR order
    V2 = np.random.default_rng(2024).uniform(-1.0, 1.0, len(I))
    ctx = pkg.Context(0)
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    B = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, True) if aat else A
    plan = pkg.CPlan(ctx, A, B)
    for _ in range(warmup):
        plan.spgemm()
    # (a) warm full pass
    full = []
    for _ in range(passes):
        plan.spgemm()
        full.append(ctx.timings()["spgemm_wall_ms"])
    steps = ctx.timings()
    dV = torch.from_numpy(V2[order]).to("cuda")
    torch.cuda.synchronize()

    def refresh():
        A.set_values_device(dV, "row")
        if aat:
            B.set_values_device(dV, "col")

    first = _ms(refresh, ctx)                                                   # (b) first call: maps built
    plan.step3()
    # correctness: (c)'s C against a fresh pipeline on the new values, bit for bit (compared on the device: cage15's C is ~11 GB)
    def c_on_device(p):
        i = p.info()
        rp = torch.empty(i["row_end"] - i["row_begin"] + 1, dtype=torch.int32, device="cuda")
        ci = torch.empty(i["nnz_c"], dtype=torch.int32, device="cuda")
        cv = torch.empty(i["nnz_c"], dtype=torch.float64, device="cuda")
        p.export_csr_device(rp.data_ptr(), ci.data_ptr(), cv.data_ptr())
        ctx.synchronize()
        return rp, ci, cv.view(torch.int64)

    got = c_on_device(plan)
    fA = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V2)
    fB = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V2, True) if aat else fA
    fresh = pkg.CPlan(ctx, fA, fB)
    fresh.spgemm()
    want = c_on_device(fresh)
    same = all(torch.equal(x, y) for x, y in zip(got, want))
    nnz_c = int(got[1].numel())
    del got, want
    torch.cuda.empty_cache()
    fresh.close()
    fA.close()
    if fB is not fA:
        fB.close()
    if not same:
        raise SystemExit(f"{name}: C after set_values_device + step3 differs from a fresh pipeline on the new values")
    for _ in range(warmup):
        refresh()
        plan.step3()
    steady = [_ms(refresh, ctx) for _ in range(passes)]                         # (b) steady state
    numeric, s3 = [], []
    for _ in range(passes):                                                     # (c)
        numeric.append(_ms(lambda: (refresh(), plan.step3()), ctx))
        s3.append(ctx.timings()["step3_ms"])
    # the refresh kernel's device time (per-kernel events; a loop of its own: the events cost a little host time)
    ctx.set_kernel_profiling(True)
    ctx.reset_kernel_stats()
    for _ in range(passes):
        refresh()
    ctx.synchronize()
    ks = ctx.kernel_stats()
    ctx.set_kernel_profiling(False)
    k = ks["vals_refresh_kernel<double>"]
    kernel_ms = k["total_ms"] / k["calls"] * (2 if aat else 1)                 # per refresh of the pass (two tilings for A*A^T)
    entries = A.nnz + (B.nnz if aat else 0)
    out = dict(workload=name, product="A*A^T" if aat else "A^2", nnz=int(A.nnz), ntiles=int(A.ntiles), entries_per_tile=A.nnz / max(A.ntiles, 1),
               nnz_c=int(nnz_c), a_full_pass=_stats(full), full_pass_steps_ms={k_: steps[k_] for k_ in ("step1_ms", "step2_ms", "step3_ms")},
               b_set_values_first_ms=first, b_set_values_steady=_stats(steady), c_numeric_pass=_stats(numeric), c_step3_ms=_stats(s3),
               refresh_kernel_ms=kernel_ms, refresh_kernel_compulsory_TBps=COMPULSORY_B[8] * entries / (kernel_ms * 1e-3) / 1e12,
               refresh_kernel_moved_TBps=MOVED_B[8] * entries / (kernel_ms * 1e-3) / 1e12, c_checked_bit_exact=True)
    plan.close()
    A.close()
    if aat:
        B.close()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated workload names (default: all five)")
    ap.add_argument("--out", default="", help="also write the results as JSON here")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("numeric_pass: no GPU (this tool measures on the device only)")
    pkg = g.load_package()
    standins = importlib.import_module("pem_spgemm_amd.standins")
    only = set(filter(None, a.only.split(",")))
    res = []
    for name, aat in WORKLOADS:
        if only and name not in only:
            continue
        r = run(pkg, standins, torch, name, aat, a.passes, a.warmup)
        res.append(r)
        print(f"{r['workload']:>14} {r['product']:>5}  nnz {r['nnz']:>9}  (a) full pass {r['a_full_pass']['median_ms']:8.3f} ms  "
              f"(b) set_values first {r['b_set_values_first_ms']:8.3f} ms, steady {r['b_set_values_steady']['median_ms']:7.3f} ms  "
              f"(c) numeric pass {r['c_numeric_pass']['median_ms']:8.3f} ms (step 3 {r['c_step3_ms']['median_ms']:.3f})  "
              f"refresh kernel {r['refresh_kernel_ms'] * 1e3:8.1f} us = {r['refresh_kernel_compulsory_TBps']:.2f} TB/s at 28 B/entry "
              f"({r['refresh_kernel_moved_TBps']:.2f} at 32)", flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(passes=a.passes, warmup=a.warmup, results=res), f, indent=1)


if __name__ == "__main__":
    main()
