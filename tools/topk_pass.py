"""Select top-k on the device (pem_tiled_select_topk) against the torch route on the same machine.

    python tools/topk_pass.py [--passes 7] [--warmup 2] [--only webbase-1M^2,cage15] [--ks 4,32,256] [--out result.json]

Per workload (seeded stand-ins, fp64: the webbase-1M stand-in's A^2 as a tiling by pem_tiled_from_cplan, and cage15's A), per k and per
dim (rows, cols), order largest; host clock around work that ends in a device synchronisation, min and median over --passes after
--warmup; kernel device times from the library's per-kernel events:
  device   S.select_topk(k, "largest", dim).
  torch    the route a caller had before: S.export_csr() (to the host) -> the triple on the device -> per-line ranking in torch (three
           stable sorts: by -x, by NaN class, by line; the rank is the position minus the line's first position) -> the kept triple in
           input order -> pem_tiled_from_coo_device.  Its stages are timed apart (export + upload, ranking, from_coo_device); it runs
           max(1, passes // 2) times after one warm-up.
Before any timing the two results are compared, array for array (every pem_tiled_info field but the timings, all twelve arrays).
fast path: the share of the non-empty line groups (16 rows or columns) in which no line has more than k entries -- the groups the
mask kernel finishes from the tiles' masks alone, without reading an entry.
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

DEFAULT = ("webbase-1M^2", "cage15")
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
        if hasattr(out, "close"):
            out.close()
    return round(min(ts), 4), round(statistics.median(ts), 4)


def _kernels(ctx, fn):
    ctx.reset_kernel_stats()
    ctx.set_kernel_profiling(True)
    out = fn()
    ctx.synchronize()
    ctx.set_kernel_profiling(False)
    st = ctx.kernel_stats()
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


def torch_route(torch, pkg, ctx, S, k, dim, times=None):
    """the kept triple by torch, as a tiling; times (a dict) receives the stages' milliseconds"""
    dev = torch.device("cuda", 0)
    t0 = time.perf_counter()
    rp, ci, v = S.export_csr()
    rp_d, J, V = torch.from_numpy(rp).to(dev), torch.from_numpy(ci).to(dev), torch.from_numpy(v).to(dev)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    n = V.numel()
    I = torch.repeat_interleave(torch.arange(S.rows, device=dev, dtype=torch.int32), (rp_d[1:] - rp_d[:-1]).to(torch.int64), output_size=n)
    line = (I if dim == "rows" else J).to(torch.int64)
    nan = torch.isnan(V)
    key = torch.where(nan, torch.zeros_like(V), -V) + 0.0            # largest: by -x ascending, -0.0 folded; the NaNs apart
    o = torch.sort(key, stable=True).indices                           # (the triple is in (row, column) order: the index inside
    o = o[torch.sort(nan[o].to(torch.int8), stable=True).indices]      # a line ascends already, and stable sorts keep it)
    o = o[torch.sort(line[o], stable=True).indices]
    sl = line[o]
    nl = S.rows if dim == "rows" else S.cols
    start = torch.cumsum(torch.bincount(sl, minlength=nl), 0) - torch.bincount(sl, minlength=nl)
    rank = torch.arange(n, device=dev) - start[sl]
    keep = torch.zeros(n, dtype=torch.bool, device=dev)
    keep[o] = rank < k
    kI, kJ, kV = I[keep].contiguous(), J[keep].contiguous(), V[keep].contiguous()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    R = pkg.Tiled.from_coo_device(ctx, S.rows, S.cols, kV.numel(), kI.data_ptr(), kJ.data_ptr(), kV.data_ptr())
    ctx.synchronize()
    t3 = time.perf_counter()
    if times is not None:
        for name, ms in (("export_upload_ms", t1 - t0), ("ranking_ms", t2 - t1), ("from_coo_device_ms", t3 - t2)):
            times.setdefault(name, []).append(ms * 1e3)
    return R


def fast_path_share(rp, ci, rows, cols, k, dim):
    n = np.diff(rp) if dim == "rows" else np.bincount(ci, minlength=cols)
    pad = (-len(n)) % 16
    grp = np.pad(n, (0, pad)).reshape(-1, 16)
    live = grp.sum(1) > 0
    return round(float(((grp.max(1) <= k) & live).sum() / max(1, live.sum())), 4), int(live.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="")
    ap.add_argument("--ks", default="4,32,256")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pkg = g.load_package()
    standins = importlib.import_module("pem_spgemm_amd.standins")
    import torch
    torch.cuda.is_available()
    names = a.only.split(",") if a.only else list(DEFAULT)
    ks = [int(x) for x in a.ks.split(",")]
    results = {}
    for name in names:
        base = name[:-2] if name.endswith("^2") else name
        rows, cols, I, J, V = standins.make(base, 1.0)
        ctx = pkg.Context(0)
        A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
        S, plan = A, None
        if name.endswith("^2"):
            plan = pkg.CPlan(ctx, A, A)
            plan.spgemm()
            S = pkg.Tiled.from_cplan(plan)
        rp, ci, _ = S.export_csr()
        r = dict(rows=S.rows, cols=S.cols, nnz=S.nnz, ntiles=S.ntiles, longest_row=int(np.diff(rp).max()),
                 longest_col=int(np.bincount(ci, minlength=S.cols).max()))
        print(f"{name}: {S.rows} x {S.cols}, nnz {S.nnz}, tiles {S.ntiles}, longest row {r['longest_row']}, longest column {r['longest_col']}", flush=True)
        for dim in ("rows", "cols"):
            S.select_topk(1, "largest", dim).close()   # (the column schedule is built once and stays with S)
            for k in ks:
                share, groups = fast_path_share(rp, ci, S.rows, S.cols, k, dim)
                R = S.select_topk(k, "largest", dim)
                W = torch_route(torch, pkg, ctx, S, k, dim)
                equal = _same_tiling(R, W)
                kept, kept_tiles = R.nnz, R.ntiles
                R.close()
                W.close()
                dmin, dmed = _timed(lambda: S.select_topk(k, "largest", dim), ctx, a.passes, a.warmup)
                kern = _kernels(ctx, lambda: S.select_topk(k, "largest", dim))
                stages = {}
                tmin, tmed = _timed(lambda: torch_route(torch, pkg, ctx, S, k, dim, stages), ctx, max(1, a.passes // 2), 1)
                stages = {n: round(statistics.median(v[1:] or v), 3) for n, v in stages.items()}
                mask_ms = round(sum(v for n, v in kern.items() if n.startswith("topk_")), 4)
                x = dict(k=k, dim=dim, kept=kept, kept_tiles=kept_tiles, equal=equal, fast_path_share=share, line_groups=groups,
                         device_ms_min=dmin, device_ms_median=dmed, mask_kernel_ms=mask_ms, kernels_ms=round(sum(kern.values()), 4),
                         kernels=kern, torch_ms_min=tmin, torch_ms_median=tmed, torch_stages_ms=stages)
                r[f"{dim}_k{k}"] = x
                print(f"{name:>14} {dim} k {k:>3}: kept {kept:>10} of {S.nnz}, equal {equal}, fast path {share:.3f} of {groups} groups | device "
                      f"min {dmin:.3f} median {dmed:.3f} ms (mask kernel {mask_ms:.3f}, all kernels {x['kernels_ms']:.3f}) | torch route min "
                      f"{tmin:.1f} median {tmed:.1f} ms (export + upload {stages['export_upload_ms']:.1f}, ranking {stages['ranking_ms']:.1f}, "
                      f"from_coo_device {stages['from_coo_device_ms']:.1f}) | ranking + from_coo_device / device "
                      f"{(stages['ranking_ms'] + stages['from_coo_device_ms']) / dmed:.1f}x", flush=True)
        results[name] = r
        if S is not A:
            S.close()
        if plan is not None:
            plan.close()
        A.close()
        ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
