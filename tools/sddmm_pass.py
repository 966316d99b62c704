"""The sampled dense-dense product on the device (pem_tiled_set_values_sddmm) against the plan route and torch.
    python tools/sddmm_pass.py [--passes 10] [--warmup 2] [--only webbase-1M-r2,...] [--ks 4,16,64,128] [--out result.json]
Per workload (seeded stand-ins: the numpy webbase-1M stand-in A, its A^2 as a tiling by pem_tiled_from_cplan, cage15 A; fp64 and
fp32), before any timing: at k = 5 the values of S.sddmm(X, Y) are compared bit for bit with route (a), the exported C of
CPlan(Xt, Ytt, mask=S) with Xt / Ytt the dense tilings of X / Y^T, under plus_times and min_plus (zero signs under min excepted).
Route (a) runs on a slice of tile rows: step 1 of a plan lists every tile-level product of its operands before the mask filters
them, tile_rows x tile_cols of them for dense operands -- 3.9e9 for a matrix of a million rows, past the int32 range of the pair
arrays -- so the plan covers the first PLAN_PRODUCTS / tile_cols tile rows (a plan's tile-row range), the check compares those rows,
and the slice's share of the entries is recorded with its time; the whole matrix takes tile_rows / slice such plans.
Then, medians over --passes after --warmup, for each k:
  the in-place call under plus_times and min_plus: kernel device time (the library's per-kernel events) and host clock (launch to a
  context synchronise);
  (a) for k <= 16, the plan route: the warm repeat pass of the masked plan over the slice alone (steps 1-3), and apart from it
      the two dense conversions a new X, Y costs for the whole matrix (the conv_ms of the two tilings, built from device arrays);
  (b) torch on the same pattern: (X[I] * Y[J]).sum(1), event time, where its nnz x k intermediate fits the budget below, and
      torch.sparse.sampled_addmm where this torch build runs it on the device (the reason is recorded otherwise).
Bytes: the compulsory traffic -- X and Y once each, the tiling's structure once per column chunk (1 byte per entry, 8 per tile,
the line pointers), the values written twice and the vals_t map read once -- as a fraction of 8 TB/s over the kernel time; and
apart from it the gathered bytes 2 * nnz * k * value_bytes, which the caches serve in part, so that a cache-served rate is not read
as an HBM one.  The bytes of X and Y are printed beside each row: below the 256 MiB last-level cache they stay resident between
passes.
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

DEFAULT = ("webbase-1M-r2", "webbase-1M-r2^2", "cage15")
PLAN_PRODUCTS = 1 << 27     # tile-level products one plan of route (a) may list
GATHER_BUDGET = 24 << 30   # bytes of torch's nnz x k intermediates (three of them live at once) above which (b) is skipped


def _chunks(k):
    w = 4 if k <= 4 else 8 if k <= 8 else 16
    return (k + w - 1) // w


def _wall(fn, ctx, passes, warmup):
    ts = []
    for _ in range(warmup + passes):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts[warmup:])


def _kernel_ms(ctx, fn, passes, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(passes):
        ctx.reset_kernel_stats()
        ctx.set_kernel_profiling(True)
        fn()
        ctx.synchronize()
        ctx.set_kernel_profiling(False)
        ts.append(sum(v["total_ms"] for v in ctx.kernel_stats().values()))
    return statistics.median(ts)


def _events(torch, fn, passes, warmup):
    for _ in range(warmup):
        fn()
    ev = []
    for _ in range(passes):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ev.append(e0.elapsed_time(e1))
    return statistics.median(ev)


def _bytes(S, vb, k):
    structure = S.nnz + 8 * S.ntiles + 4 * (S.tile_rows + 1)
    return int(vb * k * (S.rows + S.cols) + structure * max(_chunks(k), 1) + S.nnz * (2 * vb + 4))


def _frac(nbytes, ms):
    return round(nbytes / (ms * 1e-3) / 8.0e12, 4) if ms > 0 else 0.0


def _same(got, want, minmax):
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    ok = (got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want))
    if minmax:
        ok |= (got == 0) & (want == 0)
    return bool(ok.all())


def _dense_tilings(pkg, torch, ctx, S, X, Y):
    """Xt (rows x k) and Ytt (k x cols, Y^T) storing every element, from device arrays; returns them and their conversion ms"""
    k = X.shape[1]
    dt = np.dtype(S.dtype)

    def build(n, M, transpose):
        ii = torch.arange(n, dtype=torch.int32, device="cuda").repeat_interleave(k)
        cc = torch.arange(k, dtype=torch.int32, device="cuda").repeat(n)
        v = M.contiguous().view(-1)
        torch.cuda.synchronize()
        if transpose:
            return pkg.Tiled.from_coo_device(ctx, k, n, n * k, cc.data_ptr(), ii.data_ptr(), v.data_ptr(), dtype=dt)
        return pkg.Tiled.from_coo_device(ctx, n, k, n * k, ii.data_ptr(), cc.data_ptr(), v.data_ptr(), dtype=dt)

    Xt, Ytt = build(S.rows, X, False), build(S.cols, Y, True)
    return Xt, Ytt, Xt.conv_ms + Ytt.conv_ms


def one_matrix(pkg, torch, ctx, S, ks, passes, warmup):
    vb = S.value_bytes
    tdt = getattr(torch, S.dtype.name)
    r = dict(rows=S.rows, cols=S.cols, nnz=S.nnz, ntiles=S.ntiles, entries_per_tile=round(S.nnz / max(S.ntiles, 1), 2), dtype=S.dtype.name)
    rng = np.random.default_rng(5)

    def block(n, k):
        return torch.from_numpy(rng.standard_normal((n, k)).astype(S.dtype)).cuda()

    # the check first: route (a) at k = 5, bit for bit
    X, Y = block(S.rows, 5), block(S.cols, 5)
    Xt, Ytt, _ = _dense_tilings(pkg, torch, ctx, S, X, Y)
    equal = {}
    T = int(min(S.tile_rows, max(1, PLAN_PRODUCTS // max(S.tile_cols, 1))))   # route (a)'s slice: tile rows [0, T)
    nr = min(S.rows, 16 * T)
    for s in ("plus_times", "min_plus"):
        R = S.sddmm(X, Y, s)
        p = pkg.CPlan(ctx, Xt, Ytt, 0, T, mask=S, semiring=s)
        p.spgemm()
        (rp, ci, v), (crp, cci, cv) = R.export_csr(), p.export_csr()
        n = int(rp[nr])
        equal[s] = bool(np.array_equal(rp[:nr + 1], crp) and np.array_equal(ci[:n], cci) and _same(v[:n], cv, s == "min_plus"))
        p.close()
        R.close()
    Xt.close()
    Ytt.close()
    r["equal_to_plan_route"] = equal
    r["plan_route_slice"] = dict(tile_rows=T, of_tile_rows=S.tile_rows, entries=int(rp[nr]), plans_for_the_whole_matrix=-(-S.tile_rows // T))
    I = torch.from_numpy(np.repeat(np.arange(S.rows, dtype=np.int64), np.diff(rp))).cuda()
    J = torch.from_numpy(ci.astype(np.int64)).cuda()
    R = S.sddmm(X, Y)   # the tiling the in-place calls refresh (the first call builds its vals_t map)
    r["timing"] = {}
    for k in ks:
        X, Y = block(S.rows, k), block(S.cols, k)
        t = dict(xy_bytes=int(vb * k * (S.rows + S.cols)), gathered_bytes=int(2 * S.nnz * k * vb), bytes=_bytes(S, vb, k))
        for s in ("plus_times", "min_plus"):
            f = (lambda s=s: R.set_values_sddmm(X, Y, s))
            km = _kernel_ms(ctx, f, passes, warmup)
            t[s] = dict(kernel_ms=round(km, 4), wall_ms=round(_wall(f, ctx, passes, warmup), 4), hbm_frac=_frac(t["bytes"], km))
        if k <= 16:   # (a)
            Xt, Ytt, conv = _dense_tilings(pkg, torch, ctx, S, X, Y)
            p = pkg.CPlan(ctx, Xt, Ytt, 0, T, mask=S)
            p.spgemm()
            t["plan_route_slice_warm_pass_ms"] = round(_wall(lambda: p.spgemm(), ctx, passes, warmup), 4)
            t["plan_route_conversions_ms"] = round(conv, 4)
            p.close()
            Xt.close()
            Ytt.close()
        if 3 * S.nnz * k * vb <= GATHER_BUDGET:   # (b)
            try:
                t["torch_gather_ms"] = round(_events(torch, lambda: (X[I] * Y[J]).sum(1), passes, warmup), 4)
            except Exception as ex:
                t["torch_gather_ms"] = f"{type(ex).__name__}: {ex}"[:200]
        else:
            t["torch_gather_ms"] = f"skipped: three nnz x k intermediates exceed {GATHER_BUDGET >> 30} GiB"
        torch.cuda.empty_cache()
        try:
            A = torch.sparse_csr_tensor(torch.from_numpy(rp.astype(np.int64)), torch.from_numpy(ci.astype(np.int64)),
                                        torch.zeros(S.nnz, dtype=tdt), size=(S.rows, S.cols)).cuda()
            Yt = Y.t()
            t["torch_sampled_addmm_ms"] = round(_events(torch, lambda: torch.sparse.sampled_addmm(A, X, Yt, beta=0.0), passes, warmup), 4)
            del A
        except Exception as ex:   # (not every torch build runs it on the device)
            t["torch_sampled_addmm_ms"] = f"{type(ex).__name__}: {ex}"[:200]
        torch.cuda.empty_cache()
        r["timing"][str(k)] = t
    R.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="")
    ap.add_argument("--ks", default="4,16,64,128")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pkg = g.load_package()
    standins = importlib.import_module("pem_spgemm_amd.standins")
    import torch
    torch.cuda.is_available()
    names = a.only.split(",") if a.only else list(DEFAULT)
    ks = [int(x) for x in a.ks.split(",")]
    stream = torch.cuda.Stream()   # (torch's default stream is the null stream: the context and torch share this one instead)
    torch.cuda.set_stream(stream)
    ctx = pkg.Context(0, stream=stream.cuda_stream)
    results = {}
    for name in names:
        base = name[:-2] if name.endswith("^2") else name
        rows, cols, I, J, V = standins.make(base, 1.0)
        for dt in (np.float64, np.float32):
            A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=dt)
            S = A
            if name.endswith("^2"):
                plan = pkg.CPlan(ctx, A, A)
                plan.spgemm()
                S = pkg.Tiled.from_cplan(plan)
                plan.close()
            key = f"{name} {np.dtype(dt).name}"
            r = one_matrix(pkg, torch, ctx, S, ks, a.passes, a.warmup)
            results[key] = r
            print(f"{key:>24} nnz {r['nnz']:>10} tiles {r['ntiles']:>9} ({r['entries_per_tile']} entries per tile) | equal to the plan route "
                  f"{r['equal_to_plan_route']}", flush=True)
            sl = r["plan_route_slice"]
            print(f"{'':>24} plan route on tile rows [0, {sl['tile_rows']}) of {sl['of_tile_rows']}: {sl['entries']} entries", flush=True)
            for k, t in r["timing"].items():
                line = f"{'':>24} k={k:>3} X+Y {t['xy_bytes'] / 2**20:.0f} MiB, gathered {t['gathered_bytes'] / 1e6:.0f} MB"
                for s in ("plus_times", "min_plus"):
                    e = t[s]
                    line += f" | {s} {e['kernel_ms']:.3f} ms (wall {e['wall_ms']:.3f}, {e['hbm_frac']:.2f} of 8 TB/s)"
                if "plan_route_slice_warm_pass_ms" in t:
                    line += (f" | plan route warm pass {t['plan_route_slice_warm_pass_ms']:.3f} ms for 1 of {sl['plans_for_the_whole_matrix']} slices"
                             f" + conversions {t['plan_route_conversions_ms']:.3f} ms")
                for key2, label in (("torch_gather_ms", "torch gather"), ("torch_sampled_addmm_ms", "sampled_addmm")):
                    v = t[key2]
                    line += f" | {label} {v:.3f} ms" if isinstance(v, float) else f" | {label}: {v}"
                print(line, flush=True)
            if S is not A:
                S.close()
            A.close()
            if a.out:   # (after every workload: a run cut short keeps what it measured)
                with open(a.out, "w") as f:
                    json.dump(results, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
