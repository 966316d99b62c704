"""The sampled sparse product on the device (pem_tiled_sampled_mxm / pem_tiled_set_values_sampled_mxm) against the masked plan.
    python tools/sampled_pass.py [--passes 20] [--warmup 3] [--only webbase-1M-r2,...] [--out result.json]
Workloads (seeded stand-ins, fp64 and fp32):
  webbase-1M-r2        S = A, the product A * A            (the mask is far sparser than the product)
  webbase-1M-r2^2      S = A^2 (pem_tiled_from_cplan), the product A * A   (the mask IS the product's pattern)
  webbase-1M-r2 tri    triangle counting on the symmetrised stand-in: L o (L * L^T) under plus_pair, L the strict lower triangle
  cage15               S = A, the product A * A
Before any timing the values of the call are compared bit for bit with the exported C of the masked plan C<S> = A * B where the
plan stores an entry, and with the semiring's start value elsewhere.
Then, medians over --passes after --warmup, the two lane layouts alternating inside every pass (PEM_SAMPLED_LPT = 64: a wave per
pattern tile, 16: four pattern tiles per wave):
  the in-place refresh: kernel device time (the library's per-kernel events) and host clock (launch to a context synchronise);
  the builder (a new tiling: payload copy, kernel, derive_tiled), host clock;
  the plan route: the warm repeat pass of the masked plan (steps 1-3), host clock, and apart from it the B.transpose() the route
  needs where the product is A * B^T (the call reads B's rows instead).
Bytes: the compulsory traffic of the refresh -- the pattern's structure (8 bytes per tile key, 4 per tile offset, 1 per entry), the
values written twice and the vals_t map read once -- is printed as a fraction of 8 TB/s over the kernel time next to the gathered
bytes (per matched tile pair two tile ids, per pair and entry two records and, per common k, two values), which the caches serve
in part: the kernel is bound by those gathers and by the searches, not by the stream.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as g  # noqa: E402

DEFAULT = ("webbase-1M-r2", "webbase-1M-r2^2", "webbase-1M-r2 tri", "cage15")
LAYOUTS = (64, 16)
START = {"plus_times": 0.0, "plus_pair": 0.0}


def _wall_once(fn, ctx):
    ctx.synchronize()
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _kernel_once(fn, ctx):
    ctx.reset_kernel_stats()
    ctx.set_kernel_profiling(True)
    fn()
    ctx.synchronize()
    ctx.set_kernel_profiling(False)
    return sum(v["total_ms"] for k, v in ctx.kernel_stats().items() if k.startswith("sampled_kernel"))


def _alternating(measure, passes, warmup):
    """{layout: median} of measure() with the layouts alternating inside every pass"""
    ts = {l: [] for l in LAYOUTS}
    for i in range(warmup + passes):
        for l in LAYOUTS:
            os.environ["PEM_SAMPLED_LPT"] = str(l)
            v = measure()
            if i >= warmup:
                ts[l].append(v)
    os.environ.pop("PEM_SAMPLED_LPT", None)
    return {l: round(statistics.median(v), 4) for l, v in ts.items()}


def _same(got, want):
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    return bool(((got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want))).all())


def one_workload(pkg, ctx, S, A, B, tb, semiring, passes, warmup):
    """B is the call's B (transpose_b = tb)"""
    vb = A.value_bytes
    r = dict(rows=S.rows, cols=S.cols, s_nnz=S.nnz, s_tiles=S.ntiles, entries_per_tile=round(S.nnz / max(S.ntiles, 1), 2), a_nnz=A.nnz,
             b_nnz=B.nnz, dtype=A.dtype.name, semiring=semiring, transpose_b=bool(tb), flop=int(pkg.flop_count(ctx, A, B)) if not tb else None)
    # the plan route: a materialised B, the masked plan, a warm pass
    t_tr = None
    Bp = B
    if tb:
        t_tr = statistics.median(_wall_once(lambda: B.transpose().close(), ctx) for _ in range(5))
        Bp = B.transpose()
        r["flop"] = int(pkg.flop_count(ctx, A, Bp))
    plan = pkg.CPlan(ctx, A, Bp, mask=S, semiring=semiring)
    plan.spgemm()
    crp, cci, cv = plan.export_csr()
    r["plan_nnz"] = int(len(cv))
    # the check first, in both layouts
    srp, sci, _ = S.export_csr()
    skeys = np.repeat(np.arange(S.rows, dtype=np.int64), np.diff(srp)) * S.cols + sci
    stored = np.isin(skeys, np.repeat(np.arange(S.rows, dtype=np.int64), np.diff(crp)) * S.cols + cci)
    equal = {}
    for l in LAYOUTS:
        os.environ["PEM_SAMPLED_LPT"] = str(l)
        R = S.sampled_mxm(A, B, semiring, transpose_b=tb)
        v = R.export_csr()[2]
        equal[str(l)] = _same(v[stored], cv) and _same(v[~stored], np.full(int((~stored).sum()), START[semiring], v.dtype))
        R.close()
    os.environ.pop("PEM_SAMPLED_LPT", None)
    r["equal_to_masked_plan"] = equal
    R = S.sampled_mxm(A, B, semiring, transpose_b=tb)
    R.set_values_sampled_mxm(A, B, semiring, transpose_b=tb)   # (the first refresh builds the vals_t map)
    refresh = (lambda: R.set_values_sampled_mxm(A, B, semiring, transpose_b=tb))
    r["refresh_kernel_ms"] = _alternating(lambda: _kernel_once(refresh, ctx), passes, warmup)
    r["refresh_wall_ms"] = _alternating(lambda: _wall_once(refresh, ctx), passes, warmup)
    r["build_wall_ms"] = _alternating(lambda: _wall_once(lambda: S.sampled_mxm(A, B, semiring, transpose_b=tb).close(), ctx), max(passes // 2, 3), 1)
    ts = [_wall_once(plan.spgemm, ctx) for _ in range(warmup + passes)][warmup:]
    r["masked_plan_warm_pass_ms"] = round(statistics.median(ts), 4)
    r["transpose_ms"] = None if t_tr is None else round(t_tr, 4)
    r["stream_bytes"] = int(12 * S.ntiles + S.nnz * (1 + 2 * vb + 4))
    best = min(r["refresh_kernel_ms"].values())
    r["stream_frac_of_8TBs"] = round(r["stream_bytes"] / (best * 1e-3) / 8.0e12, 4) if best > 0 else 0.0
    R.close()
    plan.close()
    if Bp is not B:
        Bp.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--dtypes", default="float64,float32")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pkg = g.load_package()
    standins = importlib.import_module("pem_spgemm_amd.standins")
    import torch
    torch.cuda.is_available()
    names = a.only.split(",") if a.only else list(DEFAULT)
    stream = torch.cuda.Stream()   # (the context and torch share one stream, as in the other pass tools)
    torch.cuda.set_stream(stream)
    ctx = pkg.Context(0, stream=stream.cuda_stream)
    results = {}
    for name in names:
        base = name.split(" ")[0].replace("^2", "")
        rows, cols, I, J, V = standins.make(base, 1.0)
        for dt in [np.dtype(x) for x in a.dtypes.split(",")]:
            keep = []
            if name.endswith(" tri"):   # the strict lower triangle of the symmetrised pattern
                I64, J64 = np.asarray(I, np.int64), np.asarray(J, np.int64)
                k = np.unique(np.concatenate([I64 * cols + J64, J64 * cols + I64]))
                k = k[k // cols > k % cols]
                L = pkg.Tiled.from_coo(ctx, rows, cols, (k // cols).astype(np.int32), (k % cols).astype(np.int32), np.ones(len(k)), dtype=dt)
                S, A, B, tb, sem = L, L, L, True, "plus_pair"
                keep = [L]
            else:
                A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=dt)
                S, B, tb, sem = A, A, False, "plus_times"
                keep = [A]
                if "^2" in name:
                    plan = pkg.CPlan(ctx, A, A)
                    plan.spgemm()
                    S = pkg.Tiled.from_cplan(plan)
                    plan.close()
                    keep.append(S)
            key = f"{name} {dt.name}"
            r = one_workload(pkg, ctx, S, A, B, tb, sem, a.passes, a.warmup)
            if name.endswith(" tri"):
                per_row = S.sampled_mxm(A, B, sem, transpose_b=True).reduce("plus", "rows")
                ctx.synchronize()
                r["triangles"] = int(round(float(per_row.double().sum().item())))
            results[key] = r
            print(f"{key:>28} S nnz {r['s_nnz']:>10} tiles {r['s_tiles']:>9} ({r['entries_per_tile']} per tile) flop(A*B) {r['flop']} plan nnz "
                  f"{r['plan_nnz']} | equal to the masked plan {r['equal_to_masked_plan']}", flush=True)
            rk, rw, bw = r["refresh_kernel_ms"], r["refresh_wall_ms"], r["build_wall_ms"]
            tr = "" if r["transpose_ms"] is None else f" + B.transpose() {r['transpose_ms']:.3f} ms"
            print(f"{'':>28} {sem} refresh kernel 64: {rk[64]:.4f} ms, 16: {rk[16]:.4f} ms | wall 64: {rw[64]:.4f}, 16: {rw[16]:.4f} | build wall 64: "
                  f"{bw[64]:.3f}, 16: {bw[16]:.3f} | masked plan warm pass {r['masked_plan_warm_pass_ms']:.4f} ms{tr} | stream bytes "
                  f"{r['stream_bytes'] / 1e6:.1f} MB = {r['stream_frac_of_8TBs']:.3f} of 8 TB/s", flush=True)
            for t in keep:
                t.close()
            if a.out:   # (after every workload: a run cut short keeps what it measured)
                with open(a.out, "w") as f:
                    json.dump(results, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
