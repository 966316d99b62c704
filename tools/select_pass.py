"""Select on the device (pem_tiled_select, its positional refresh) against the host route.

    python tools/select_pass.py [--passes 10] [--warmup 2] [--only webbase-1M,...] [--out result.json]

Per workload (seeded stand-ins; C = A^2 as a tiling by pem_tiled_from_cplan; host clock around work that ends in a device
synchronisation, medians over --passes; kernel device times from the library's per-kernel events):
  (1) abs_gt at the median |value| of C (keeps about half), (2) value_ne:0, (3) tril:-1 -- each against the host route: export C
      (pem_tiled_export_csr), filter in numpy, pem_tiled_from_csr.  Before any timing the device result is compared, array for array,
      with pem_tiled_from_coo of tests/selectref.py's result on the exported C.
  (4) the positional refresh pem_tiled_set_values_from_select of (3), against a fresh select; compared first as well.
Bytes: the select kernels' nominal traffic -- C's row masks (32 B per tile), rowcolidx (1 B) and vals read, R's payload written (tile
key, offset and source tile: 16 B per tile; rowcolidx, tile-head scan and value per entry) -- as a fraction of 8 TB/s over the time of
the sel_* kernels alone and over every kernel of the call (the scans and derive_tiled included).
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
import selectref as sel  # noqa: E402

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


def _timed(fn, ctx, passes, warmup, close=True):
    ts = []
    for i in range(warmup + passes):
        t, out = _ms(fn, ctx)
        if i >= warmup:
            ts.append(t)
        if close and hasattr(out, "close"):
            out.close()
    return statistics.median(ts)


def _kernels(ctx, fn):
    ctx.reset_kernel_stats()
    ctx.set_kernel_profiling(True)
    out = fn()
    ctx.synchronize()
    ctx.set_kernel_profiling(False)
    st = ctx.kernel_stats()
    if hasattr(out, "close"):
        out.close()
    return {k: round(v["total_ms"], 4) for k, v in st.items()}


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


def _gbs_frac(nbytes, ms):
    return round(nbytes / (ms * 1e-3) / 8.0e12, 4) if ms > 0 else 0.0


def one_op(pkg, ctx, C, coo, op, thunk, passes, warmup):
    rows, cols = C.rows, C.cols
    R = C.select(op, thunk)
    want = pkg.Tiled.from_coo(ctx, rows, cols, *sel.select(*coo, op, thunk))
    equal = _same_tiling(R, want)
    want.close()

    def host():
        r, ci, v = C.export_csr()
        I = np.repeat(np.arange(rows, dtype=np.int32), np.diff(r))
        m = sel.keep(op, I, ci, v, thunk)
        return pkg.Tiled.from_csr(ctx, rows, cols, np.concatenate([[0], np.cumsum(np.bincount(I[m], minlength=rows))]), ci[m], v[m])

    dev = _timed(lambda: C.select(op, thunk), ctx, passes, warmup)
    kern = _kernels(ctx, lambda: C.select(op, thunk))
    sel_ms = round(sum(v for k, v in kern.items() if k.startswith("sel_")), 4)
    all_ms = round(sum(kern.values()), 4)
    hst = _timed(host, ctx, max(1, passes // 5), 1)
    nbytes = 32 * C.ntiles + 9 * C.nnz + 16 * R.ntiles + 13 * R.nnz
    out = dict(op=op, thunk=float(thunk), nnz=R.nnz, ntiles=R.ntiles, equal=equal, device_ms=round(dev, 4), sel_kernels_ms=sel_ms,
               kernels_ms=all_ms, kernels=kern, bytes=int(nbytes), hbm_frac_sel_kernels=_gbs_frac(nbytes, sel_ms),
               hbm_frac_all_kernels=_gbs_frac(nbytes, all_ms), host_route_ms=round(hst, 3))
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
        rp, ci, v = C.export_csr()
        coo = (np.repeat(np.arange(rows, dtype=np.int32), np.diff(rp)), ci, v)
        med = float(np.median(np.abs(v))) if len(v) else 0.0
        r = dict(rows=rows, nnz_a=A.nnz, nnz_c=C.nnz, ntiles_c=C.ntiles)
        for key, op, thunk in (("abs_gt_median", "abs_gt", med), ("value_ne_0", "value_ne", 0.0), ("tril_m1", "tril", -1)):
            R, r[key] = one_op(pkg, ctx, C, coo, op, thunk, a.passes, a.warmup)
            if key != "tril_m1":
                R.close()
        # (4) refresh of tril:-1 after new values of C, against a fresh select
        C.set_values(np.random.default_rng(1).normal(size=C.nnz))
        R.set_values_from_select(C)   # (first call: builds the map)
        F = C.select("tril", -1)
        r["refresh_equal"] = _same_tiling(R, F)
        F.close()
        r["refresh_ms"] = round(_timed(lambda: R.set_values_from_select(C), ctx, a.passes, a.warmup), 4)
        r["refresh_kernels_ms"] = round(sum(_kernels(ctx, lambda: R.set_values_from_select(C)).values()), 4)
        r["fresh_select_ms"] = round(_timed(lambda: C.select("tril", -1), ctx, a.passes, a.warmup), 4)
        R.close()
        results[name] = r
        line = f"{name:>14} C nnz {C.nnz:>10} tiles {C.ntiles:>9}"
        for key in ("abs_gt_median", "value_ne_0", "tril_m1"):
            x = r[key]
            line += (f" | {x['op']}:{x['thunk']:.3g} kept {x['nnz']}, equal {x['equal']}, {x['device_ms']:.3f} ms (sel kernels "
                     f"{x['sel_kernels_ms']:.3f}, {x['hbm_frac_sel_kernels']:.2f} of 8 TB/s; all kernels {x['kernels_ms']:.3f}, "
                     f"{x['hbm_frac_all_kernels']:.2f}) vs host {x['host_route_ms']:.1f} ms")
        line += (f" | refresh {r['refresh_ms']:.3f} ms (kernels {r['refresh_kernels_ms']:.3f}, equal {r['refresh_equal']}) vs fresh select "
                 f"{r['fresh_select_ms']:.3f} ms")
        print(line, flush=True)
        C.close()
        plan.close()
        A.close()
        ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
