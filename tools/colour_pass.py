"""Graph colouring on the device (pem_tiled_colour / pem_colour_order) against the host route it replaces, and what the reordering buys.

    python tools/colour_pass.py [--passes 7] [--warmup 2] [--scale 1.0] [--out profiles/colour_pass.json]

The matrix: trsv_pass's -- the seeded webbase-1M stand-in's off-diagonal pattern, symmetrised, standard normal values, a dominant
diagonal -- in fp64.  Two colourings of it on the device, warm, the median of --passes host clocks around a call (the colouring waits
by itself; the others end in a context synchronise):
  hashed    A.colour(seed=0): the priorities are a hash of the vertex number
  natural   A.colour(priority=0 everywhere): ties go to the lower index, tools/trsv_pass.py's natural-order greedy colouring
Per colouring: the colour time with symmetric=False (row and column walk) and with symmetric=True (the pattern is symmetric: the same
colours from the row walk alone), rounds, colours, time per round, the time inside the rounds' kernels; colour_order; extract(p, p);
and on the reordered matrix the lower triangle's levels (trsv_info), one solve, and one ILU(0) refresh
(F.set_values_from_ilu0).  Alongside, on the same matrix in the
same run: the host's greedy_colouring (tools/trsv_pass.py) with the colours and levels it yields -- the natural colouring must equal
it -- the unreordered matrix's levels, solve and refresh, and one mxv, the floor of a round (a round reads every entry's position
once, as an mxv does, but no value).
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as g  # noqa: E402
from trsv_pass import _median, greedy_colouring, symmetric_problem  # noqa: E402


def _stats(t):
    med, lo, hi = t
    return dict(median=round(med, 4), min=round(lo, 4), max=round(hi, 4))


def downstream(torch, ctx, M, passes, warmup):
    """levels of the lower triangle, one solve, one ILU(0) refresh"""
    n = M.rows
    b = torch.from_numpy(np.random.default_rng(11).standard_normal(n)).cuda()
    x = torch.empty_like(b)
    r = dict(levels=M.trsv_info("lower")["levels"], launches=M.trsv_info("lower")["launches"])
    M.trsv(b, "lower", out=x)
    r["solve_ms"] = _stats(_median(lambda: M.trsv(b, "lower", out=x), ctx, passes, warmup))
    F = M.ilu0()
    r["ilu0_levels"] = F.ilu0_info()["levels"]
    r["ilu0_refresh_ms"] = _stats(_median(lambda: F.set_values_from_ilu0(M), ctx, max(3, passes // 2), 1))
    F.close()
    return r


def measure(pkg, torch, ctx, A, label, priority, passes, warmup):
    r = {}
    runs = {}
    for sym in (False, True):
        c, nc, rounds = A.colour(seed=0, priority=priority, symmetric=sym)
        runs[sym] = c
        t = _stats(_median(lambda: A.colour(seed=0, priority=priority, symmetric=sym, out=c), ctx, passes, warmup))
        key = "colour_symmetric_ms" if sym else "colour_ms"
        r[key] = t
        r[key.replace("_ms", "_us_per_round")] = round(1e3 * t["median"] / max(1, rounds), 3)
        # the rounds' kernels alone (event pairs around every launch): what the call spends outside them is launches and read-backs
        ctx.reset_kernel_stats()
        ctx.set_kernel_profiling(True)
        A.colour(seed=0, priority=priority, symmetric=sym, out=c)
        ctx.synchronize()
        ks = [v for k, v in ctx.kernel_stats().items() if k.startswith("colour_round_kernel")]
        ctx.set_kernel_profiling(False)
        r[key.replace("_ms", "_kernels_ms")] = round(sum(v["total_ms"] for v in ks), 4)
        r.update(colours=nc, rounds=rounds)
    ctx.synchronize()
    torch.cuda.synchronize()
    r["symmetric_equals_general"] = bool(torch.equal(runs[False], runs[True]))
    c = runs[False]
    p, off = pkg.colour_order(ctx, c, nc)
    r["colour_order_ms"] = _stats(_median(lambda: pkg.colour_order(ctx, c, nc), ctx, passes, warmup))
    keep = []

    def extract():
        for R in keep:
            R.close()
        keep[:] = [A.extract(p, p)]

    r["extract_ms"] = _stats(_median(extract, ctx, passes, warmup))
    R = keep[0]
    sizes = np.diff(off.cpu().numpy())
    r["colour_sizes"] = dict(largest=int(sizes.max()), smallest=int(sizes.min()))
    r["reordered"] = downstream(torch, ctx, R, passes, warmup)
    R.close()
    d = r["reordered"]
    print(f"{label:>8}: {nc} colours in {rounds} rounds | colour {r['colour_ms']['median']:.3f} ms ({r['colour_us_per_round']:.1f} us/round, "
          f"kernels {r['colour_kernels_ms']:.3f} ms), symmetric=True {r['colour_symmetric_ms']['median']:.3f} ms "
          f"({r['colour_symmetric_us_per_round']:.1f} us/round, kernels {r['colour_symmetric_kernels_ms']:.3f} ms), same colours "
          f"{r['symmetric_equals_general']} | colour_order {r['colour_order_ms']['median']:.3f} ms | extract(p, p) {r['extract_ms']['median']:.3f} ms | "
          f"reordered: {d['levels']} levels, solve {d['solve_ms']['median']:.3f} ms, ILU(0) refresh {d['ilu0_refresh_ms']['median']:.3f} ms", flush=True)
    return r, c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pkg = g.load_package()
    standins = importlib.import_module("pem_spgemm_amd.standins")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("colour_pass: no GPU (this tool measures on the device only)")
    stream = torch.cuda.Stream()   # (torch's default stream is the null stream: the context and torch share this one instead)
    torch.cuda.set_stream(stream)
    ctx = pkg.Context(0, stream=stream.cuda_stream)
    n, I, J, V = symmetric_problem(standins, a.scale)
    results = dict(workload=f"webbase-1M stand-in (scale {a.scale}), symmetrised pattern, dominant diagonal", passes=a.passes, warmup=a.warmup,
                   n=n, nnz=len(I))
    A = pkg.Tiled.from_coo(ctx, n, n, I, J, V)
    # the floor of a round: one mxv (row orientation, and the column orientation the general colouring also walks)
    x = torch.from_numpy(np.random.default_rng(3).standard_normal(n)).cuda()
    y = torch.empty_like(x)
    A.mxv(x, out=y), A.mxv(x, transpose=True, out=y)
    results["mxv_ms"] = _stats(_median(lambda: A.mxv(x, out=y), ctx, a.passes, a.warmup))
    results["mxv_transpose_ms"] = _stats(_median(lambda: A.mxv(x, transpose=True, out=y), ctx, a.passes, a.warmup))
    print(f"n {n} nnz {len(I)} | mxv {results['mxv_ms']['median']:.3f} ms, transposed {results['mxv_transpose_ms']['median']:.3f} ms", flush=True)
    results["unreordered"] = downstream(torch, ctx, A, a.passes, a.warmup)
    d = results["unreordered"]
    print(f"unreordered: {d['levels']} levels, solve {d['solve_ms']['median']:.3f} ms, ILU(0) refresh {d['ilu0_refresh_ms']['median']:.3f} ms", flush=True)
    results["hashed"], _ = measure(pkg, torch, ctx, A, "hashed", None, a.passes, a.warmup)
    zeros = torch.zeros(n, dtype=torch.int32, device="cuda")
    results["natural"], c_nat = measure(pkg, torch, ctx, A, "natural", zeros, a.passes, a.warmup)
    # the host route: the Python loop on the exported pattern, then the same order and extract
    t0 = time.perf_counter()
    colour = greedy_colouring(n, I.astype(np.int64), J.astype(np.int64))
    host_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    ph = np.argsort(colour, kind="stable").astype(np.int32)
    sort_s = time.perf_counter() - t0
    R = A.extract(ph, ph)
    results["host_greedy"] = dict(host_seconds=round(host_s, 3), argsort_seconds=round(sort_s, 3), colours=int(colour.max()) + 1,
                                  levels=R.trsv_info("lower")["levels"],
                                  equals_device_natural=bool(np.array_equal(colour.astype(np.int32), c_nat.cpu().numpy())))
    R.close()
    h = results["host_greedy"]
    print(f"host greedy_colouring {h['host_seconds']:.2f} s (+ argsort {h['argsort_seconds']:.3f} s): {h['colours']} colours, {h['levels']} levels, "
          f"equals the device's natural colouring {h['equals_device_natural']}", flush=True)
    for k in ("hashed", "natural"):
        r = results[k]
        r["device_route_ms"] = round(r["colour_symmetric_ms"]["median"] + r["colour_order_ms"]["median"], 3)
        r["host_over_device"] = round(1e3 * (host_s + sort_s) / r["device_route_ms"], 1)
    A.close()
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
