"""The Krylov solvers on the device (pem_krylov_*) on two orderings of one problem, against their floor and against the loop a user
would write in torch.

    python tools/krylov_pass.py [--passes 7] [--warmup 2] [--scale 1.0] [--iters 20] [--out profiles/krylov_pass.json]

The matrix: trsv_pass's -- the seeded webbase-1M stand-in's off-diagonal pattern, symmetrised -- made symmetric in VALUE as well
(one standard normal value per pair) with a positive dominant diagonal (row abs sum + 1 + U[0, 1)): symmetric positive definite,
fp64.  Two orderings of it: natural, and coloured (the library's colouring and extract, Tiled.reorder_by_colour), where the ILU(0)
solves have few levels.
Per ordering and per configuration -- CG with none / diag / LU (the ILU(0) factor), BiCGStab with LU -- the time PER ITERATION:
a solve of exactly --iters iterations (rtol = 0, max_iters = check_every = --iters: one read-back, the status max_iters), the
host clock around it, divided by --iters; warm passes, then the median of --passes with min and max kept.  The start of a solve
(one mxv, two or three kernels) is inside that time.  Alongside, in the same run:
  mxv floor    the same number of mxv calls alone (iters + 1 for CG, 2 iters + 1 for BiCGStab), per iteration
  own kernels  one profiled solve: the krylov_* kernels' summed time per iteration (kernel_stats), the bytes they move per iteration
               (every vector read or written once per kernel that touches it) and the GB/s that gives
  torch route  the CG of INTEGRATION.md section 3y written in torch: the library's mxv (and lu_solve), torch.dot, scalars kept on the
               device (no .item()), --iters iterations, one synchronise at the end; none and LU
and the iterations CG needs to rtol = 1e-8 with none, diag and LU.
"""
import argparse
import importlib
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
    fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _stat(fn, ctx, passes, warmup, per):
    ts = [_wall(fn, ctx) / per for _ in range(warmup + passes)][warmup:]
    return dict(median=round(statistics.median(ts), 5), min=round(min(ts), 5), max=round(max(ts), 5))


def spd_problem(standins, scale, seed=7):
    """(n, I, J, V): the stand-in's off-diagonal pattern on both sides, one normal value per pair, a positive dominant diagonal"""
    rows, cols, I, J, _ = standins.make("webbase-1M", scale)
    n = max(rows, cols)
    I, J = np.asarray(I, np.int64), np.asarray(J, np.int64)
    off = I != J
    lo, hi = np.minimum(I[off], J[off]), np.maximum(I[off], J[off])
    key = np.unique(hi * n + lo)
    hi, lo = key // n, key % n
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(len(hi))
    s = np.zeros(n)
    np.add.at(s, hi, np.abs(v))
    np.add.at(s, lo, np.abs(v))
    d = s + 1.0 + rng.random(n)
    ar = np.arange(n, dtype=np.int64)
    return (n, np.concatenate([hi, lo, ar]).astype(np.int32), np.concatenate([lo, hi, ar]).astype(np.int32), np.concatenate([v, v, d]))


def own_bytes(method, precond, n, vb):
    """bytes the solver's own kernels move per iteration: vectors read + written, per kernel"""
    if method == "cg":
        vecs = 2 + 6 + 3   # dot(p, q); update: x r p q in, x r out; p: r|z p in, p out
        if precond == "diag":
            vecs += 2       # minv in the update and in the p kernel
        if precond == "lu":
            vecs += 2       # the second dot reads r and z
    else:
        vecs = 2 + 3 + 2 + 8 + 4   # dot(rhat, v); s: r v in, s out; ts: s t in; xr: x y z s t rhat in, x r out; p: r p v in, p out
        if precond == "diag":
            vecs += 4               # minv in and z out in the s kernel, minv in and y out in the p kernel
    return vecs * n * vb


def torch_cg(torch, A, F, b, iters):
    """section 3y's route as a CG: the library's mxv / lu_solve, torch's dots and axpys, device scalars"""
    x = torch.zeros_like(b)
    q, z, w = torch.empty_like(b), torch.empty_like(b), torch.empty_like(b)
    A.mxv(x, out=q)
    r = b - q
    if F is not None:
        F.lu_solve(r, out=z, work=w)
    else:
        z = r
    p = z.clone()
    rz = torch.dot(r, z)
    for _ in range(iters):
        A.mxv(p, out=q)
        alpha = rz / torch.dot(p, q)
        x.add_(alpha * p)
        r.sub_(alpha * q)
        if F is not None:
            F.lu_solve(r, out=z, work=w)
        rzn = torch.dot(r, z)
        p.mul_(rzn / rz).add_(z)
        rz = rzn
    return x, torch.dot(r, r)


def measure(pkg, torch, ctx, A, label, a):
    n, vb = A.rows, A.value_bytes
    b = torch.from_numpy(np.random.default_rng(11).standard_normal(n)).cuda()
    r = dict(n=n, nnz=A.nnz)
    t0 = time.perf_counter()
    F = A.ilu0()
    ctx.synchronize()
    r["ilu0_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    lo, up = F.trsv_info("lower"), F.trsv_info("upper")
    r["trsv"] = dict(levels=[lo["levels"], up["levels"]], launches=[lo["launches"], up["launches"]])
    D = A.select("diag", 0)
    minv = 1 / D.reduce("plus")
    D.close()
    torch.cuda.current_stream().synchronize()
    y = torch.empty_like(b)
    x = torch.empty_like(b)
    for nm in (a.iters + 1, 2 * a.iters + 1):
        r[f"mxv_floor_{nm}_calls_ms_per_iter"] = _stat(lambda: [A.mxv(b, out=y) for _ in range(nm)], ctx, a.passes, a.warmup, a.iters)
    for method, pc in (("cg", "none"), ("cg", "diag"), ("cg", "lu"), ("bicgstab", "lu")):
        K = pkg.Krylov(A, method=method, precond={"none": None, "diag": "diag", "lu": F}[pc], max_iters=a.iters, check_every=a.iters, rtol=0.0)
        m = minv if pc == "diag" else None
        last = {}

        def run():
            x.zero_()
            last["info"] = K.solve(b, x=x, minv=m)[1]

        e = dict(ms_per_iter=_stat(run, ctx, a.passes, a.warmup, a.iters))
        info = last["info"]
        e.update(status=info["status"], iters=info["iters"], launches=info["launches"], readbacks=info["readbacks"])
        ctx.synchronize()
        ctx.set_kernel_profiling(True)
        ctx.reset_kernel_stats()
        run()
        ctx.synchronize()
        stats = ctx.kernel_stats()
        ctx.set_kernel_profiling(False)
        own = {k: s for k, s in stats.items() if k.startswith("krylov_")}
        own_ms = sum(s["total_ms"] for s in own.values()) / a.iters
        nbytes = own_bytes(method, pc, n, vb)
        e["own_kernels"] = dict(ms_per_iter=round(own_ms, 5), calls={k: s["calls"] for k, s in own.items()}, bytes_per_iter=int(nbytes),
                                gb_per_s=round(nbytes / (own_ms * 1e-3) / 1e9, 1) if own_ms > 0 else None)
        e["other_kernels_ms_per_iter"] = round(sum(s["total_ms"] for k, s in stats.items() if not k.startswith("krylov_")) / a.iters, 5)
        r[f"{method}_{pc}"] = e
        K.close()
        print(f"{label:>9} {method:>8} {pc:>4}: {e['ms_per_iter']['median']:.4f} ms/iter ({e['status']} after {e['iters']}), own kernels "
              f"{own_ms:.4f} ms/iter = {e['own_kernels']['gb_per_s']} GB/s, other kernels {e['other_kernels_ms_per_iter']:.4f} ms/iter", flush=True)
    for pc, Fp in (("none", None), ("lu", F)):
        out = {}

        def run_torch():
            out["x"], out["rr"] = torch_cg(torch, A, Fp, b, a.iters)

        r[f"torch_cg_{pc}"] = dict(ms_per_iter=_stat(run_torch, ctx, a.passes, a.warmup, a.iters), rr=float(out["rr"].item()))
        print(f"{label:>9} torch cg {pc:>4}: {r[f'torch_cg_{pc}']['ms_per_iter']['median']:.4f} ms/iter", flush=True)
    r["iterations_to_1e-8"] = {}
    for pc in ("none", "diag", "lu"):
        xs, info = A.solve(b, method="cg", precond={"none": None, "diag": minv, "lu": F}[pc], max_iters=500, rtol=1e-8)
        r["iterations_to_1e-8"][f"cg_{pc}"] = dict(iters=info["iters"], status=info["status"], rnorm_rel=float(np.sqrt(info["rr"] / info["bb"])))
    xs, info = A.solve(b, method="bicgstab", precond=F, max_iters=500, rtol=1e-8)
    r["iterations_to_1e-8"]["bicgstab_lu"] = dict(iters=info["iters"], status=info["status"], rnorm_rel=float(np.sqrt(info["rr"] / info["bb"])))
    print(f"{label:>9} iterations to 1e-8: {r['iterations_to_1e-8']}", flush=True)
    F.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pkg = g.load_package()
    standins = importlib.import_module("pem_spgemm_amd.standins")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("krylov_pass: no GPU (this tool measures on the device only)")
    stream = torch.cuda.Stream()   # (torch's default stream is the null stream: the context and torch share this one instead)
    torch.cuda.set_stream(stream)
    ctx = pkg.Context(0, stream=stream.cuda_stream)
    n, I, J, V = spd_problem(standins, a.scale)
    results = dict(workload=f"webbase-1M stand-in (scale {a.scale}), symmetrised pattern, symmetric values, positive dominant diagonal, fp64",
                   passes=a.passes, warmup=a.warmup, iters=a.iters)
    S = pkg.Tiled.from_coo(ctx, n, n, I, J, V)
    results["natural"] = measure(pkg, torch, ctx, S, "natural", a)
    t0 = time.perf_counter()
    R, perm, offsets = S.reorder_by_colour(seed=0, symmetric=True)
    ctx.synchronize()
    results["colouring"] = dict(colours=int(len(offsets) - 1), device_ms=round((time.perf_counter() - t0) * 1e3, 1))
    S.close()
    results["coloured"] = measure(pkg, torch, ctx, R, "coloured", a)
    R.close()
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
