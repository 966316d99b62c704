"""Independent sets and aggregation on the device (pem_tiled_mis / pem_tiled_aggregate) against the host route they replace, and one
whole coarsening level.

    python tools/aggregate_pass.py [--passes 7] [--warmup 2] [--scale 1.0] [--grid 1000] [--out profiles/aggregate_pass.json]

The matrices, in fp64: colour_pass's -- the seeded webbase-1M stand-in's off-diagonal pattern, symmetrised, standard normal values, a
dominant diagonal -- and the --grid x --grid five-point grid with its vertices shuffled (seeded), the same values.  Per matrix, warm,
the median of --passes host clocks around a call (every call here waits by itself):
  A.aggregate and A.mis at distance 1 and 2, with symmetric=False (row and column walk) and symmetric=True (both patterns are
  symmetric: the same result from the row walk alone): time, rounds, time per round, the time inside the kernels (event pairs);
  A.colour(seed=0) beside them: one colouring round is the same walk, so it is the yardstick of a round -- a distance-2 round is two
  walks;
  the host route: export_csr, the model's vectorised numpy equivalent (two-hop maxima by np.maximum.reduceat over the CSR, the two
  assignment passes the same way), upload -- and whether its aggregates equal the device's;
  the whole level: aggregate(symmetric=True), prolongator, transpose, the two plans with their products and the two from_cplan --
  with the coarse size and nnz(Ac) / nnz(A).
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
from trsv_pass import _median, symmetric_problem, with_diagonal  # noqa: E402

IN_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
INT32_MAX = 2 ** 31 - 1


def _stats(t):
    med, lo, hi = t
    return dict(median=round(med, 4), min=round(lo, 4), max=round(hi, 4))


def shuffled_grid(k, seed=5):
    """(n, I, J, V): the k x k five-point grid, both directions of every edge, the vertices renumbered by a seeded permutation"""
    v = np.arange(k * k, dtype=np.int64).reshape(k, k)
    a = np.concatenate([v[:, :-1].ravel(), v[:-1, :].ravel()])
    b = np.concatenate([v[:, 1:].ravel(), v[1:, :].ravel()])
    p = np.random.default_rng(seed).permutation(k * k)
    a, b = p[a], p[b]
    return with_diagonal(k * k, np.concatenate([a, b]), np.concatenate([b, a]), np.random.default_rng(seed + 1))


def fmix32(h):
    h = h.astype(np.uint32)
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def host_aggregate(n, rowptr, colidx, seed=0):
    """(agg, naggregates, rounds) of the contract on a symmetric CSR pattern, vectorised: the host route's middle step"""
    rowptr = rowptr.astype(np.int64)
    full = np.flatnonzero(np.diff(rowptr) > 0)
    starts = rowptr[full]

    def spread(val):   # out[v] = max(val[v], max of val over v's row)
        out = val.copy()
        if len(colidx):
            out[full] = np.maximum(out[full], np.maximum.reduceat(val[colidx], starts))
        return out

    prio = fmix32(np.arange(n, dtype=np.uint64) + np.uint64((seed * 0x9E3779B9) & 0xFFFFFFFF))
    beat = ((prio.astype(np.uint64) << np.uint64(31)) | (np.uint64(INT32_MAX) - np.arange(n, dtype=np.uint64))) + np.uint64(1)
    key, rounds = beat.copy(), 0
    while rounds < n:
        m = spread(spread(key))
        und = (key != 0) & (key != IN_KEY)
        new = key.copy()
        new[und & (m == IN_KEY)] = 0
        new[und & (m == key)] = IN_KEY
        key = new
        rounds += 1
        if not np.any((key != 0) & (key != IN_KEY)):
            break
    roots = np.flatnonzero(key == IN_KEY)
    agg = np.full(n, -1, np.int32)
    agg[roots] = np.arange(len(roots), dtype=np.int32)
    for _ in range(2):
        cand = np.where(agg >= 0, beat, np.uint64(0))
        best = np.zeros(n, np.uint64)
        if len(colidx):
            best[full] = np.maximum.reduceat(cand[colidx], starts)
        take = (agg < 0) & (best != 0)
        winner = INT32_MAX - ((best[take] - np.uint64(1)) & np.uint64(INT32_MAX)).astype(np.int64)
        nxt = agg.copy()
        nxt[take] = agg[winner]
        agg = nxt
    return agg, len(roots), rounds


def kernels_ms(ctx, fn, prefixes):
    """the time inside the named kernels of one call (event pairs around every launch)"""
    ctx.reset_kernel_stats()
    ctx.set_kernel_profiling(True)
    fn()
    ctx.synchronize()
    ks = [v for k, v in ctx.kernel_stats().items() if k.startswith(prefixes)]
    ctx.set_kernel_profiling(False)
    return round(sum(v["total_ms"] for v in ks), 4)


def measure(pkg, torch, ctx, label, n, I, J, V, passes, warmup):
    A = pkg.Tiled.from_coo(ctx, n, n, I, J, V)
    r = dict(n=n, nnz=len(I))
    for sym in (False, True):
        tag = "_symmetric" if sym else ""
        c, nc, crounds = A.colour(seed=0, symmetric=sym)
        t = _stats(_median(lambda: A.colour(seed=0, symmetric=sym, out=c), ctx, passes, warmup))
        r["colour" + tag] = dict(ms=t, rounds=crounds, colours=nc, us_per_round=round(1e3 * t["median"] / max(1, crounds), 2))
        for d in (1, 2):
            s, count, rounds = A.mis(distance=d, symmetric=sym)
            t = _stats(_median(lambda: A.mis(distance=d, symmetric=sym, out=s), ctx, passes, warmup))
            r[f"mis{d}" + tag] = dict(ms=t, rounds=rounds, count=count, us_per_round=round(1e3 * t["median"] / max(1, rounds), 2),
                                      kernels_ms=kernels_ms(ctx, lambda: A.mis(distance=d, symmetric=sym, out=s), ("mis_round_kernel",)))
        agg, roots, nagg, rounds = A.aggregate(symmetric=sym)
        t = _stats(_median(lambda: A.aggregate(symmetric=sym, out=agg), ctx, passes, warmup))
        r["aggregate" + tag] = dict(ms=t, rounds=rounds, naggregates=nagg, us_per_round=round(1e3 * t["median"] / max(1, rounds), 2),
                                    rounds_kernels_ms=kernels_ms(ctx, lambda: A.aggregate(symmetric=sym, out=agg), ("mis_round_kernel",)),
                                    assign_kernels_ms=kernels_ms(ctx, lambda: A.aggregate(symmetric=sym, out=agg), ("aggregate_assign_kernel",)))
    ctx.synchronize()
    torch.cuda.synchronize()
    dev_agg = agg.cpu().numpy()
    sizes = np.bincount(dev_agg, minlength=1)
    r["aggregate_sizes"] = dict(largest=int(sizes.max()), smallest=int(sizes.min()), mean=round(float(sizes.mean()), 2))
    # the host route: export, the vectorised model, upload
    t0 = time.perf_counter()
    rp, ci, _ = A.export_csr()
    t1 = time.perf_counter()
    hagg, hn, hrounds = host_aggregate(n, rp, ci)
    t2 = time.perf_counter()
    up = torch.from_numpy(hagg).cuda()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    r["host_route"] = dict(export_ms=round(1e3 * (t1 - t0), 2), model_ms=round(1e3 * (t2 - t1), 2), upload_ms=round(1e3 * (t3 - t2), 2),
                           total_ms=round(1e3 * (t3 - t0), 2), equals_device=bool(np.array_equal(hagg, dev_agg) and (hn, hrounds) == (nagg, rounds)))
    r["host_over_device"] = round(r["host_route"]["total_ms"] / r["aggregate_symmetric"]["ms"]["median"], 1)
    del up
    # the whole level
    keep = []

    def level():
        for T in keep:
            T.close()
        a, _, nc, _ = A.aggregate(symmetric=True, roots=False)
        P = pkg.prolongator(ctx, a, nc)
        Pt = P.transpose()
        ap = pkg.CPlan(ctx, A, P)
        ap.spgemm()
        AP = pkg.Tiled.from_cplan(ap)
        gp = pkg.CPlan(ctx, Pt, AP)
        gp.spgemm()
        Ac = pkg.Tiled.from_cplan(gp)
        ap.close(), gp.close()
        keep[:] = [P, Pt, AP, Ac]

    t = _stats(_median(level, ctx, max(3, passes // 2), 1))
    Ac = keep[3]
    r["level"] = dict(ms=t, coarse_n=Ac.rows, coarse_nnz=Ac.nnz, nnz_ratio=round(Ac.nnz / len(I), 4))
    for T in keep:
        T.close()
    A.close()
    ag, ags, m2, c = r["aggregate"], r["aggregate_symmetric"], r["mis2_symmetric"], r["colour_symmetric"]
    print(f"{label}: n {n} nnz {len(I)} | aggregate {ag['ms']['median']:.3f} ms, symmetric=True {ags['ms']['median']:.3f} ms: {ags['naggregates']} "
          f"aggregates in {ags['rounds']} rounds ({ags['us_per_round']:.1f} us/round; rounds' kernels {ags['rounds_kernels_ms']:.3f} ms, assign "
          f"{ags['assign_kernels_ms']:.3f} ms) | mis(2) {m2['ms']['median']:.3f} ms, mis(1) {r['mis1_symmetric']['ms']['median']:.3f} ms in "
          f"{r['mis1_symmetric']['rounds']} rounds ({r['mis1_symmetric']['us_per_round']:.1f} us/round) | a colouring round {c['us_per_round']:.1f} us "
          f"({c['rounds']} rounds) | host route {r['host_route']['total_ms']:.0f} ms (export {r['host_route']['export_ms']:.0f}, model "
          f"{r['host_route']['model_ms']:.0f}, upload {r['host_route']['upload_ms']:.1f}), equal {r['host_route']['equals_device']}, "
          f"{r['host_over_device']}x | level {r['level']['ms']['median']:.2f} ms -> {r['level']['coarse_n']} x {r['level']['coarse_n']}, "
          f"nnz(Ac)/nnz(A) {r['level']['nnz_ratio']}", flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--grid", type=int, default=1000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pkg = g.load_package()
    standins = importlib.import_module("pem_spgemm_amd.standins")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("aggregate_pass: no GPU (this tool measures on the device only)")
    stream = torch.cuda.Stream()   # (torch's default stream is the null stream: the context and torch share this one instead)
    torch.cuda.set_stream(stream)
    ctx = pkg.Context(0, stream=stream.cuda_stream)
    results = dict(passes=a.passes, warmup=a.warmup, workloads={})
    work = (("webbase", f"webbase-1M stand-in (scale {a.scale}), symmetrised pattern, dominant diagonal", lambda: symmetric_problem(standins, a.scale)),
            ("grid", f"{a.grid} x {a.grid} five-point grid, vertices shuffled", lambda: shuffled_grid(a.grid)))
    for label, what, make in work:
        n, I, J, V = make()
        results["workloads"][label] = dict(workload=what, **measure(pkg, torch, ctx, label, n, I, J, V, a.passes, a.warmup))
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
