"""Apply and scale on the device (pem_tiled_apply, pem_tiled_scale, their refreshes) against the routes they replace.

    python tools/apply_pass.py [--passes 10] [--warmup 2] [--only webbase-1M,...] [--out result.json]

Per workload (seeded stand-ins; C = A^2 as a tiling by pem_tiled_from_cplan; host clock around work that ends in a device
synchronisation, medians over --passes; kernel device times from the library's per-kernel events).  Every timed result is first
compared, array for array, with pem_tiled_from_coo of tests/applyref.py's result on the exported C.
  builds     apply(abs), apply(powi:2), scale(times, r, c), against
               (i)  the host route: pem_tiled_export_csr, numpy, pem_tiled_from_csr;
               (ii) for scale, the plan route: two products with diagonal tilings (made once, outside the clock) and two
                    pem_tiled_from_cplan.
  refreshes  set_values_from_apply, set_values_from_scale, against
               (iii) the best device route without them: the values of C and per-entry row and column index tensors (int32) on the
                    device, made once, V' = f(V) resp. r[I] * V * c[J] in torch, then pem_tiled_set_values_device -- on a context that shares
                    torch's stream, so nothing waits in between.
Bytes: the kernels' nominal traffic as a fraction of 8 TB/s -- apply reads and writes both value arrays (4 values per entry); scale
reads the value, 1 B of rowcolidx and 4 B of vmap_t and writes two values.
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
import applyref as ap  # noqa: E402

DEFAULT = ("webbase-1M", "webbase-1M-r2", "scircuit")
ARRAYS = ("tile_keys", "tile_nnz_ptr", "masks", "rowptr", "rowcolidx", "vals", "masks_t", "tile_rowptr", "tile_colidx", "tile_colptr",
          "tile_rowidx", "tile_offsets")
INFO = ("rows", "cols", "nnz", "tile_rows", "tile_cols", "ntiles", "value_bytes")


def _ms(fn, ctx):
    ctx.synchronize()
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _timed(fn, ctx, passes, warmup):
    ts = []
    for i in range(warmup + passes):
        t, out = _ms(fn, ctx)
        if i >= warmup:
            ts.append(t)
        for x in out if isinstance(out, (list, tuple)) else (out,):
            if hasattr(x, "close"):
                x.close()
    return round(statistics.median(ts), 4)


def _kernels(ctx, fn, prefix):
    ctx.reset_kernel_stats()
    ctx.set_kernel_profiling(True)
    out = fn()
    ctx.synchronize()
    ctx.set_kernel_profiling(False)
    st = ctx.kernel_stats()
    if hasattr(out, "close"):
        out.close()
    return round(sum(v["total_ms"] for k, v in st.items() if k.startswith(prefix)), 4), round(sum(v["total_ms"] for v in st.values()), 4)


def _same_tiling(x, y):
    if any(getattr(x, k) != getattr(y, k) for k in INFO):
        return False
    for k in ARRAYS:
        a, b = x.array(k), y.array(k)
        if a.dtype.kind == "f":
            a, b = a.view(np.uint64), b.view(np.uint64)
        if not np.array_equal(a, b):
            return False
    return True


def _same_vals_t(ctx, x, y, probe):
    """vals_t through its reader: mxv with transpose"""
    import torch
    a, b = x.mxv(probe, transpose=True), y.mxv(probe, transpose=True)
    ctx.synchronize()
    return torch.equal(a.view(torch.int64), b.view(torch.int64))


def _frac(nbytes, ms):
    return round(nbytes / (ms * 1e-3) / 8.0e12, 4) if ms > 0 else 0.0


def workload(pkg, torch, name, standins, passes, warmup):
    rows, cols, I, J, V = standins.make(name, 1.0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = pkg.Context(0, stream=stream.cuda_stream)
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    plan = pkg.CPlan(ctx, A, A)
    plan.spgemm()
    C = pkg.Tiled.from_cplan(plan)
    rp, ci, v = C.export_csr()
    n, nnz, nt = C.rows, C.nnz, C.ntiles
    eI = np.repeat(np.arange(n, dtype=np.int32), np.diff(rp))
    rng = np.random.default_rng(7)
    r, c = rng.uniform(0.5, 2.0, n), rng.uniform(0.5, 2.0, n)
    dr, dc, probe = (torch.from_numpy(x).cuda() for x in (r, c, rng.normal(size=n)))
    dI, dJ, dV = torch.from_numpy(eI).cuda(), torch.from_numpy(np.asarray(ci, np.int32)).cuda(), torch.from_numpy(v).cuda()
    torch.cuda.synchronize()
    res = dict(rows=n, nnz_a=A.nnz, nnz_c=nnz, ntiles_c=nt)

    def host(f):
        p, q, w = C.export_csr()
        return pkg.Tiled.from_csr(ctx, n, n, p, q, f(np.repeat(np.arange(n, dtype=np.int32), np.diff(p)), q, w))

    # ---- builds ----
    builds = (("apply_abs", lambda: C.apply("abs"), lambda i, j, w: ap.apply(w, "abs"), "apply_kernel", 32 * nnz),
              ("apply_powi2", lambda: C.apply("powi", 2), lambda i, j, w: ap.apply(w, "powi", 2), "apply_kernel", 32 * nnz),
              ("scale", lambda: C.scale(dr, dc), lambda i, j, w: ap.scale(i, j, w, r, c), "scale_kernel", 29 * nnz + 12 * nt))
    for key, dev, ref, prefix, nbytes in builds:
        R = dev()
        want = pkg.Tiled.from_coo(ctx, n, n, eI, ci, ref(eI, ci, v))
        equal = _same_tiling(R, want) and _same_vals_t(ctx, R, want, probe)
        R.close()
        want.close()
        k_ms, all_ms = _kernels(ctx, dev, prefix)
        res[key] = dict(equal=equal, device_ms=_timed(dev, ctx, passes, warmup), kernel_ms=k_ms, all_kernels_ms=all_ms, bytes=int(nbytes),
                        hbm_frac_kernel=_frac(nbytes, k_ms))
        res[key]["host_route_ms"] = _timed(lambda: host(ref), ctx, max(1, passes // 5), 1)
    Dr = pkg.Tiled.from_coo(ctx, n, n, np.arange(n), np.arange(n), r)
    Dc = pkg.Tiled.from_coo(ctx, n, n, np.arange(n), np.arange(n), c)

    def plan_route():
        p1 = pkg.CPlan(ctx, Dr, C)
        p1.spgemm()
        T = pkg.Tiled.from_cplan(p1)
        p2 = pkg.CPlan(ctx, T, Dc)
        p2.spgemm()
        return pkg.Tiled.from_cplan(p2), p2, T, p1

    out = plan_route()
    S = C.scale(dr, dc)
    res["plan_route_equal"] = _same_tiling(out[0], S)
    S.close()
    for x in out:
        x.close()
    res["scale_plan_route_ms"] = _timed(plan_route, ctx, max(1, passes // 2), 1)

    # ---- refreshes ----
    C.set_values(np.random.default_rng(1).normal(size=nnz))
    rp2, ci2, v2 = C.export_csr()
    dV.copy_(torch.from_numpy(v2))
    torch.cuda.synchronize()
    Ra, Rp = C.apply("abs"), C.apply("powi", 2)
    refreshes = [("refresh_apply_abs", Ra, lambda: Ra.set_values_from_apply(C), lambda: C.apply("abs"), lambda: Ra.set_values_device(dV.abs()),
                  "apply_kernel", 32 * nnz),
                 ("refresh_apply_powi2", Rp, lambda: Rp.set_values_from_apply(C), lambda: C.apply("powi", 2), lambda: Rp.set_values_device(dV * dV),
                  "apply_kernel", 32 * nnz)]
    Rs = C.scale(dr, dc)
    refreshes.append(("refresh_scale", Rs, lambda: Rs.set_values_from_scale(C, dr, dc), lambda: C.scale(dr, dc),
                      lambda: Rs.set_values_device(dr[dI] * dV * dc[dJ]), "scale_kernel", 29 * nnz + 12 * nt))
    for key, R, refresh, fresh, torch_route, prefix, nbytes in refreshes:
        refresh()   # (first call)
        ctx.synchronize()
        F = fresh()
        equal = _same_tiling(R, F) and _same_vals_t(ctx, R, F, probe)
        torch_route()
        ctx.synchronize()
        equal_torch = _same_tiling(R, F)   # (the route's own result, for the record)
        F.close()
        k_ms, _ = _kernels(ctx, refresh, prefix)
        res[key] = dict(equal=equal, torch_route_equal=equal_torch, device_ms=_timed(refresh, ctx, passes, warmup), kernel_ms=k_ms,
                        bytes=int(nbytes), hbm_frac_kernel=_frac(nbytes, k_ms), torch_route_ms=_timed(torch_route, ctx, passes, warmup))
    for x in [t[1] for t in refreshes] + [Dr, Dc, C, plan, A]:
        x.close()
    ctx.close()
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--passes", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--only", default="")
    p.add_argument("--out", default="")
    a = p.parse_args()
    pkg = g.load_package()
    standins = importlib.import_module("pem_spgemm_amd.standins")
    import torch
    torch.cuda.is_available()
    results = {}
    for name in a.only.split(",") if a.only else list(DEFAULT):
        r = results[name] = workload(pkg, torch, name, standins, a.passes, a.warmup)
        print(f"{name}: C nnz {r['nnz_c']} tiles {r['ntiles_c']}", flush=True)
        for key in ("apply_abs", "apply_powi2", "scale"):
            x = r[key]
            print(f"  {key:>22}: equal {x['equal']}, {x['device_ms']:.3f} ms (kernel {x['kernel_ms']:.4f} ms, {x['hbm_frac_kernel']:.2f} of 8 TB/s; "
                  f"all kernels {x['all_kernels_ms']:.3f} ms)" + f" vs host route {x['host_route_ms']:.1f} ms", flush=True)
        print(f"  {'scale, plan route':>22}: equal {r['plan_route_equal']}, {r['scale_plan_route_ms']:.3f} ms", flush=True)
        for key in ("refresh_apply_abs", "refresh_apply_powi2", "refresh_scale"):
            x = r[key]
            print(f"  {key:>22}: equal {x['equal']}, {x['device_ms']:.4f} ms (kernel {x['kernel_ms']:.4f} ms, {x['hbm_frac_kernel']:.2f} of 8 TB/s) "
                  f"vs torch route {x['torch_route_ms']:.4f} ms (equal {x['torch_route_equal']})", flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
