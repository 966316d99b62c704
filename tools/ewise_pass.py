"""Element-wise combination of tilings on the device (pem_tiled_ewise, its refresh, pem_tiled_export_csr) against the host route.

    python tools/ewise_pass.py [--passes 10] [--warmup 2] [--only webbase-1M,...] [--out result.json]

Per workload (seeded stand-ins; C = A^2 as a tiling by pem_tiled_from_cplan; host clock around work that ends in a device
synchronisation, medians over --passes; kernel device times from the library's per-kernel events):
  (1) ewise(C, A, UNION, PLUS) and (2) ewise(C, A, INTERSECT, TIMES), each against the host route: export both operands
      (pem_tiled_export_csr), scipy's + or .multiply, pem_tiled_from_csr.  Before any timing the device result is compared, array for
      array, with pem_tiled_from_coo of tests/ewiseref.py's result.
  (3) the refresh pem_tiled_set_values_from_ewise of (1), against a fresh ewise.
  (4) the tiling export of C (pem_tiled_export_csr) against the plan export of the same C (pem_c_export_csr); both are compared first.
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
import ewiseref as er  # noqa: E402

DEFAULT = ("webbase-1M", "webbase-1M-r2", "scircuit")
ARRAYS = ("tile_keys", "tile_nnz_ptr", "masks", "rowptr", "rowcolidx", "vals", "masks_t", "tile_rowptr", "tile_colidx", "tile_colptr",
          "tile_rowidx", "tile_offsets")


def _ms(fn, ctx):
    ctx.synchronize()
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _timed(fn, ctx, passes, warmup, close=True):
    ts = []
    for i in range(warmup + passes):
        t, out = _ms(fn, ctx)
        if i >= warmup:
            ts.append(t)
        if close and hasattr(out, "close"):
            out.close()
    return statistics.median(ts)


def _kernel_ms(ctx, fn):
    ctx.reset_kernel_stats()
    ctx.set_kernel_profiling(True)
    out = fn()
    ctx.synchronize()
    ctx.set_kernel_profiling(False)
    st = ctx.kernel_stats()
    if hasattr(out, "close"):
        out.close()
    return round(sum(v["total_ms"] for v in st.values()), 4), {k: round(v["total_ms"], 4) for k, v in st.items()}


def _same_tiling(x, y):
    for k in ARRAYS:
        a, b = x.array(k), y.array(k)
        if a.dtype.kind == "f":
            a, b = a.view(np.uint64), b.view(np.uint64)
        if not np.array_equal(a, b):
            return False
    return True


def _coo(rp, ci, v):
    return np.repeat(np.arange(len(rp) - 1, dtype=np.int32), np.diff(rp)), ci, v


def one_op(pkg, ctx, C, A, csr_c, csr_a, op, pattern, passes, warmup):
    import scipy.sparse as sp
    rows, cols = A.rows, A.cols
    R = pkg.Tiled.ewise(C, A, op=op, pattern=pattern)
    I, J, V = er.ewise(cols, _coo(*csr_c), _coo(*csr_a), op, pattern)
    want = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    equal = _same_tiling(R, want)
    want.close()
    del I, J, V

    def host():
        c, a = C.export_csr(), A.export_csr()
        mc = sp.csr_matrix((c[2], c[1], c[0]), shape=(rows, cols))
        ma = sp.csr_matrix((a[2], a[1], a[0]), shape=(rows, cols))
        s = (mc + ma) if op == "plus" else mc.multiply(ma).tocsr()
        s.sort_indices()
        return pkg.Tiled.from_csr(ctx, rows, cols, s.indptr, s.indices, s.data)

    dev = _timed(lambda: pkg.Tiled.ewise(C, A, op=op, pattern=pattern), ctx, passes, warmup)
    kms, kern = _kernel_ms(ctx, lambda: pkg.Tiled.ewise(C, A, op=op, pattern=pattern))
    hst = _timed(host, ctx, max(1, passes // 5), 1)
    out = dict(op=op, pattern=pattern, nnz=R.nnz, ntiles=R.ntiles, equal=equal, device_ms=round(dev, 4), kernels_ms=kms, kernels=kern,
               host_route_ms=round(hst, 3))
    return R, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pkg = g.load_package()
    standins = importlib.import_module("pem_spgemm_amd.standins")
    import torch
    torch.cuda.is_available()
    names = a.only.split(",") if a.only else list(DEFAULT)
    results = {}
    for name in names:
        rows, cols, I, J, V = standins.make(name, 1.0)
        ctx = pkg.Context(0)
        A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
        plan = pkg.CPlan(ctx, A, A)
        plan.spgemm()
        C = pkg.Tiled.from_cplan(plan)
        csr_c, csr_a = C.export_csr(), A.export_csr()
        r = dict(rows=rows, nnz_a=A.nnz, nnz_c=C.nnz)
        R, r["union_plus"] = one_op(pkg, ctx, C, A, csr_c, csr_a, "plus", "union", a.passes, a.warmup)
        X, r["intersect_times"] = one_op(pkg, ctx, C, A, csr_c, csr_a, "times", "intersect", a.passes, a.warmup)
        X.close()
        # (3) refresh: after new values of A, against a fresh ewise
        A.set_values(np.random.default_rng(1).normal(size=A.nnz))
        R.set_values_from_ewise(C, A)   # (first call: builds the map)
        F = pkg.Tiled.ewise(C, A)
        r["refresh_equal"] = _same_tiling(R, F)
        F.close()
        r["refresh_ms"] = round(_timed(lambda: R.set_values_from_ewise(C, A), ctx, a.passes, a.warmup), 4)
        r["refresh_kernels_ms"], _ = _kernel_ms(ctx, lambda: R.set_values_from_ewise(C, A))
        R.close()
        # (4) tiling export against plan export of the same C (plan's C is still current: A's refresh made it stale, so run step 3)
        A.set_values(csr_a[2])
        plan.step3()
        pe = plan.export_csr()
        te = C.export_csr()
        r["export_equal"] = all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in zip(pe, te))
        r["tiled_export_ms"] = round(_timed(C.export_csr, ctx, a.passes, a.warmup, close=False), 4)
        r["tiled_export_kernels_ms"], r["tiled_export_kernels"] = _kernel_ms(ctx, C.export_csr)
        r["plan_export_ms"] = round(_timed(plan.export_csr, ctx, a.passes, a.warmup, close=False), 4)
        r["plan_export_kernels_ms"], r["plan_export_kernels"] = _kernel_ms(ctx, plan.export_csr)
        results[name] = r
        u, x = r["union_plus"], r["intersect_times"]
        print(f"{name:>14} C nnz {C.nnz:>10} A nnz {A.nnz:>9} | union plus: {u['nnz']} nnz, equal {u['equal']}, {u['device_ms']:.3f} ms "
              f"(kernels {u['kernels_ms']:.3f}) vs host {u['host_route_ms']:.1f} ms | intersect times: {x['nnz']} nnz, equal {x['equal']}, "
              f"{x['device_ms']:.3f} ms (kernels {x['kernels_ms']:.3f}) vs host {x['host_route_ms']:.1f} ms | refresh {r['refresh_ms']:.3f} ms "
              f"(kernels {r['refresh_kernels_ms']:.3f}, equal {r['refresh_equal']}) | export tiling {r['tiled_export_ms']:.3f} ms "
              f"(kernels {r['tiled_export_kernels_ms']:.3f}) vs plan {r['plan_export_ms']:.3f} ms (kernels {r['plan_export_kernels_ms']:.3f}), "
              f"equal {r['export_equal']}", flush=True)
        C.close()
        plan.close()
        A.close()
        ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
