"""The aggregation multigrid on the device (pem_amg_*) as a preconditioner of CG, against no, a diagonal and an ILU(0) preconditioner.

    python tools/amg_pass.py [--passes 3] [--warmup 1] [--n2 1000] [--n3 100] [--max-iters 4000] [--out profiles/amg_pass.json]

Workloads, fp64: the 5-point Laplacian on an n2 x n2 grid and the 7-point Laplacian on an n3^3 grid (diagonal 4 resp. 6,
off-diagonal -1), b standard normal, a zero guess.
Per workload and per preconditioner -- none, jacobi, ilu0, amg-plain, amg-smoothed (the binding's defaults: symmetric=False, seed 0,
coarse_size 40, one sweep, four coarse sweeps, omega 2/3) -- CG to rtol 1e-8: the iterations, the status and the host clock around
the solve (warm passes, then the median of --passes with min and max kept); the preconditioner's setup and, for the hierarchies,
the refresh after new values on A (the second and later refreshes; the first, which builds the refresh maps, apart).
Per hierarchy: levels, rows, nnz, operator complexity, launches per apply; one apply's wall time; ONE PROFILED APPLY split by kernel
name (the amg_* kernels against the mxv kernels); and level by level the launches of the cycle, the time of that level's three
products alone (mxv of A_l, of R_l, of P_l with accumulate, each profiled on the level's own tilings) and the share of the apply's
launches that lie below level 0 -- the figure a decision on graph capture of the cycle needs.  The amg_* kernels carry no level
in their names, so their time is given per kernel name, not per level.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402


def _wall(fn, ctx):
    ctx.synchronize()
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _stat(fn, ctx, passes, warmup):
    ts = [_wall(fn, ctx)[0] for _ in range(warmup + passes)][warmup:]
    return dict(median=round(statistics.median(ts), 4), min=round(min(ts), 4), max=round(max(ts), 4))


def grid(shape):
    """the (2 d + 1)-point Laplacian on a grid of the given shape: (n, I, J, V), int32 indices"""
    idx = np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape)
    I, J = [idx.ravel()], [idx.ravel()]
    for ax in range(len(shape)):
        a = np.take(idx, np.arange(shape[ax] - 1), axis=ax).ravel()
        b = np.take(idx, np.arange(1, shape[ax]), axis=ax).ravel()
        I += [a, b]
        J += [b, a]
    I, J = np.concatenate(I), np.concatenate(J)
    V = np.where(I == J, 2.0 * len(shape), -1.0)
    return idx.size, I.astype(np.int32), J.astype(np.int32), V


LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def _profiled(ctx, fn):
    ctx.synchronize()
    ctx.set_kernel_profiling(True)
    ctx.reset_kernel_stats()
    try:
        fn()
        ctx.synchronize()
        return {k: s for k, s in ctx.kernel_stats().items() if s["calls"]}
    finally:
        ctx.set_kernel_profiling(False)


def hierarchy_report(pkg, torch, ctx, A, M, b, a):
    info = M.info
    r = {k: info[k] for k in ("levels", "rows", "nnz", "p_nnz", "aggregate_rounds", "launches", "bytes")}
    r["operator_complexity"] = round(info["operator_complexity"], 4)
    z = torch.empty_like(b)
    r["apply_ms"] = _stat(lambda: M.apply(b, out=z), ctx, a.passes + 4, a.warmup + 1)
    stats = _profiled(ctx, lambda: M.apply(b, out=z))
    own = {k: s for k, s in stats.items() if k.startswith("amg_")}
    mxv = {k: s for k, s in stats.items() if k.startswith("mxv_kernel")}
    r["one_apply_by_kernel"] = dict(
        amg={k: dict(calls=s["calls"], ms=round(s["total_ms"], 5)) for k, s in own.items()},
        mxv=dict(calls=sum(s["calls"] for s in mxv.values()), ms=round(sum(s["total_ms"] for s in mxv.values()), 5)),
        amg_ms=round(sum(s["total_ms"] for s in own.values()), 5), kernel_ms=round(sum(s["total_ms"] for s in stats.values()), 5))
    sweeps, coarse_sweeps, L = M.opts["sweeps"], M.opts["coarse_sweeps"], info["levels"]
    per_level = []
    for l in range(L):
        A_l, P_l, R_l = M.level(l)
        e = dict(rows=info["rows"][l], launches=2 * coarse_sweeps - 1 if l + 1 == L else 4 * sweeps + 3)
        x = torch.ones(A_l.rows, dtype=torch.float64, device="cuda")
        y = torch.empty_like(x)
        A_l.mxv(x, out=y)
        e["mxv_A_ms"] = round(sum(s["total_ms"] for s in _profiled(ctx, lambda: A_l.mxv(x, out=y)).values()), 5)
        if P_l is not None:
            xc = torch.ones(P_l.cols, dtype=torch.float64, device="cuda")
            R_l.mxv(x, out=xc)
            e["mxv_R_ms"] = round(sum(s["total_ms"] for s in _profiled(ctx, lambda: R_l.mxv(x, out=xc)).values()), 5)
            P_l.mxv(xc, out=y, accumulate=True)
            e["mxv_P_ms"] = round(sum(s["total_ms"] for s in _profiled(ctx, lambda: P_l.mxv(xc, out=y, accumulate=True)).values()), 5)
        per_level.append(e)
    r["per_level"] = per_level
    r["launch_share_below_level_0"] = round(sum(e["launches"] for e in per_level[1:]) / max(1, info["launches"]), 4)
    return r


def measure(pkg, torch, ctx, label, case, a):
    n, I, J, V = case
    A = pkg.Tiled.from_coo(ctx, n, n, I, J, V)
    b = torch.from_numpy(np.random.default_rng(11).standard_normal(n)).cuda()
    o = np.lexsort((J, I))
    dv, dv2 = torch.from_numpy(V[o]).cuda(), torch.from_numpy(1.25 * V[o]).cuda()
    out = dict(n=n, nnz=int(A.nnz))
    x = torch.empty_like(b)
    for name in ("none", "jacobi", "ilu0", "amg_plain", "amg_smoothed"):
        e = {}
        minv = F = M = None
        t0 = time.perf_counter()
        if name == "jacobi":
            D = A.select("diag", 0)
            minv = 1 / D.reduce("plus")
            D.close()
            torch.cuda.current_stream().synchronize()
        elif name == "ilu0":
            F = A.ilu0()
        elif name.startswith("amg"):
            M = pkg.Amg(A, smooth=name == "amg_smoothed")
        ctx.synchronize()
        e["setup_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        if M is not None:
            e["hierarchy"] = hierarchy_report(pkg, torch, ctx, A, M, b, a)
            A.set_values_device(dv2)
            e["first_refresh_ms"] = round(_wall(M.refresh, ctx)[0], 3)
            A.set_values_device(dv)
            M.refresh()

            def refresh():
                A.set_values_device(dv)
                M.refresh()

            e["refresh_ms"] = _stat(refresh, ctx, a.passes, a.warmup)
        K = pkg.Krylov(A, method="cg", precond="diag" if minv is not None else (F or M), max_iters=a.max_iters, check_every=16, rtol=1e-8)
        last = {}

        def run():
            x.zero_()
            last["info"] = K.solve(b, x=x, minv=minv)[1]

        # (ILU(0) in the natural order of a grid runs thousands of trsv launches per iteration: one cold pass)
        e["solve_ms"] = _stat(run, ctx, 1, 0) if name == "ilu0" else _stat(run, ctx, a.passes, a.warmup)
        info = last["info"]
        e.update(iters=info["iters"], status=info["status"], launches=info["launches"], rnorm_rel=float(np.sqrt(info["rr"] / info["bb"])))
        K.close()
        for h in (F, M):
            if h is not None:
                h.close()
        out[name] = e
        say(f"{label:>8} cg {name:>12}: {e['iters']:5d} iterations ({e['status']}), solve {e['solve_ms']['median']:.2f} ms, setup "
              f"{e['setup_ms']:.2f} ms" + (f", refresh {e['refresh_ms']['median']:.2f} ms, {e['hierarchy']['levels']} levels, rows "
                                         f"{e['hierarchy']['rows']}, complexity {e['hierarchy']['operator_complexity']}, "
                                         f"{e['hierarchy']['launches']} launches per apply ({e['hierarchy']['launch_share_below_level_0']:.0%} "
                                         f"below level 0), apply {e['hierarchy']['apply_ms']['median']:.3f} ms" if M is not None else ""))
        if M is not None:
            k = e["hierarchy"]["one_apply_by_kernel"]
            say(f"{'':>8}    one apply by kernel: amg_* {k['amg_ms']:.4f} ms in {sum(v['calls'] for v in k['amg'].values())} launches, mxv "
                f"{k['mxv']['ms']:.4f} ms in {k['mxv']['calls']}; per level (rows, launches, mxv A / R / P ms): "
                + "; ".join(f"{v['rows']}, {v['launches']}, {v['mxv_A_ms']} / {v.get('mxv_R_ms', '-')} / {v.get('mxv_P_ms', '-')}"
                            for v in e["hierarchy"]["per_level"]))
    A.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n2", type=int, default=1000)
    ap.add_argument("--n3", type=int, default=100)
    ap.add_argument("--max-iters", type=int, default=4000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pkg = g.load_package()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("amg_pass: no GPU (this tool measures on the device only)")
    stream = torch.cuda.Stream()   # (torch's default stream is the null stream: the context and torch share this one instead)
    torch.cuda.set_stream(stream)
    ctx = pkg.Context(0, stream=stream.cuda_stream)
    results = dict(workload="5-point and 7-point Laplacians, fp64, CG to rtol 1e-8 from a zero guess", passes=a.passes, warmup=a.warmup,
                   max_iters=a.max_iters)
    for label, shape in ((f"grid2d_{a.n2}", (a.n2, a.n2)), (f"grid3d_{a.n3}", (a.n3, a.n3, a.n3))):
        results[label] = measure(pkg, torch, ctx, label, grid(shape), a)
        if a.out:   # (kept after every workload: a later one that runs long loses nothing)
            with open(a.out, "w") as f:
                json.dump(results, f, indent=1)
            with open(os.path.splitext(a.out)[0] + ".txt", "w") as f:
                f.write("\n".join(LINES) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
