"""Block assembly on the device (pem_tiled_concat, pem_tiled_set_values_from_concat) against the two routes that exist without it.

    python tools/concat_pass.py [--passes 10] [--warmup 2] [--only grid2x2,...] [--scale 1.0] [--out result.json]

Per workload (the webbase-1M stand-in, seeded; host clock around work that ends in a device synchronisation, medians over --passes;
kernel device times from the library's per-kernel events):
  concat     Tiled.concat(grid) on the device;
  refresh    set_values_from_concat after new values in every block (first compared with a fresh concat);
  assign     the assign route: one Tiled.assign per non-null block into a tiling of the full shape that starts empty;
  torch      the torch route: the blocks' (row, column, value) triples on the device (made once, outside the clock), shifted and
             joined by torch.cat, then pem_tiled_from_coo_device -- on a context that shares torch's stream, so nothing waits in
             between.  Its tiling is what concat's is compared with, array for array, and vals_t through mxv(transpose=True).
Workloads (A = the stand-in, n x n):
  grid2x2    [[A, A^T], [A^T, A]]
  vstack8    a vertical stack of 8 tile-row slices of A (A.extract of 8 row ranges that start at multiples of 16): A again
  offset7    [[S, 0], [0, A]] with a dense 7 x 7 block S: every row and column offset of A is 7 mod 16, each of its tiles is cut
             four ways
Bytes (fp64): the payload kernel's nominal traffic -- per entry 13 B written (value, (r << 4) | c byte, tile-head scan) and 8 B
read, per tile of the result 60 B -- as a fraction of 8 TB/s over cc_fill_kernel's time; the refresh moves 44 B per entry (the int2
map, vmap_t, the gathered value, two written).
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

DEFAULT = ("grid2x2", "vstack8", "offset7")
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
    return round(statistics.median(ts), 4)


def _kernels(ctx, fn):
    """device ms of one call by kernel name"""
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


def _same_vals_t(torch, ctx, x, y):
    """vals_t through its reader: mxv with transpose"""
    probe = torch.from_numpy(np.random.default_rng(3).normal(size=x.rows)).cuda()
    torch.cuda.synchronize()
    a, b = x.mxv(probe, transpose=True), y.mxv(probe, transpose=True)
    ctx.synchronize()
    return torch.equal(a.view(torch.int64), b.view(torch.int64))


def _frac(nbytes, ms):
    return round(nbytes / (ms * 1e-3) / 8.0e12, 4) if ms > 0 else 0.0


def _triples(torch, T):
    """a tiling's entries as device tensors (int64 rows, int64 columns, values), in CSR order"""
    rp, ci, v = T.export_csr()
    I = np.repeat(np.arange(T.rows, dtype=np.int64), np.diff(rp))
    out = torch.from_numpy(I).cuda(), torch.from_numpy(ci.astype(np.int64)).cuda(), torch.from_numpy(v).cuda()
    torch.cuda.synchronize()
    return out


def _grid(pkg, ctx, name, A):
    """(the grid as a list of lists of tilings or None, row sizes, column sizes)"""
    n = A.rows
    if name == "grid2x2":
        At = A.transpose()
        return [[A, At], [At, A]], [n, n], [n, n]
    if name == "vstack8":
        cut = [min(n, (A.tile_rows * k // 8) * 16) for k in range(9)]
        return [[A.extract(slice(cut[k], cut[k + 1]), None)] for k in range(8)], [cut[k + 1] - cut[k] for k in range(8)], [A.cols]
    if name == "offset7":
        I, J = (x.ravel().astype(np.int32) for x in np.meshgrid(np.arange(7), np.arange(7), indexing="ij"))
        S = pkg.Tiled.from_coo(ctx, 7, 7, I, J, np.random.default_rng(11).uniform(0.5, 1.5, 49))
        return [[S, None], [None, A]], [7, n], [7, A.cols]
    raise SystemExit(f"unknown workload {name}")


def workload(pkg, torch, name, coo, passes, warmup):
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = pkg.Context(0, stream=stream.cuda_stream)
    A = pkg.Tiled.from_coo(ctx, *coo)
    grid, rs, cs = _grid(pkg, ctx, name, A)
    ro, co = np.concatenate([[0], np.cumsum(rs)]), np.concatenate([[0], np.cumsum(cs)])
    rows, cols = int(ro[-1]), int(co[-1])
    cells = [(a, b, blk) for a, row in enumerate(grid) for b, blk in enumerate(row) if blk is not None]
    distinct = list({id(blk): blk for _, _, blk in cells}.values())
    trip = {id(blk): _triples(torch, blk) for blk in distinct}
    n = sum(blk.nnz for _, _, blk in cells)
    empty = pkg.Tiled.from_coo(ctx, rows, cols, [], [], [])

    def torch_route():
        P = torch.cat([trip[id(blk)][0] + int(ro[a]) for a, _, blk in cells]).to(torch.int32)
        Q = torch.cat([trip[id(blk)][1] + int(co[b]) for _, b, blk in cells]).to(torch.int32)
        V = torch.cat([trip[id(blk)][2] for _, _, blk in cells])
        return pkg.Tiled.from_coo_device(ctx, rows, cols, n, P.data_ptr(), Q.data_ptr(), V.data_ptr(), False)

    def assign_route():
        Z = empty
        for a, b, blk in cells:
            Z2 = Z.assign(blk, slice(int(ro[a]), int(ro[a + 1])), slice(int(co[b]), int(co[b + 1])))
            if Z is not empty:
                Z.close()
            Z = Z2
        return Z

    dev = lambda: pkg.Tiled.concat(grid, rs, cs)
    R, want, via_assign = dev(), torch_route(), assign_route()
    res = dict(rows=rows, cols=cols, cells=len(cells), nnz=R.nnz, ntiles=R.ntiles)
    res["equal"] = _same_tiling(R, want) and _same_vals_t(torch, ctx, R, want)
    res["assign_equal"] = _same_tiling(via_assign, want)
    want.close()
    via_assign.close()
    ks = _kernels(ctx, dev)
    nbytes = 21 * R.nnz + 60 * R.ntiles
    res["kernels_ms"] = ks
    res["concat"] = dict(device_ms=_timed(dev, ctx, passes, warmup), concat_kernels_ms=round(sum(v for k, v in ks.items() if k.startswith("cc_")), 4),
                         all_kernels_ms=round(sum(ks.values()), 4), fill_kernel_ms=round(sum(v for k, v in ks.items() if k.startswith("cc_fill")), 4),
                         bytes=int(nbytes))
    res["concat"]["hbm_frac_fill"] = _frac(nbytes, res["concat"]["fill_kernel_ms"])
    res["torch_route_ms"] = _timed(torch_route, ctx, max(2, passes // 2), 1)
    res["assign_route_ms"] = _timed(assign_route, ctx, max(2, passes // 2), 1)
    res["ratio_torch"] = round(res["torch_route_ms"] / res["concat"]["device_ms"], 2)
    res["ratio_assign"] = round(res["assign_route_ms"] / res["concat"]["device_ms"], 2)
    # ---- refresh ----
    rng = np.random.default_rng(1)
    R.set_values_from_concat(grid)   # (first call: the map)
    for blk in distinct:
        blk.set_values(rng.normal(size=blk.nnz))
    R.set_values_from_concat(grid)
    ctx.synchronize()
    F = dev()
    refresh = lambda: R.set_values_from_concat(grid)
    rk = _kernels(ctx, refresh)
    r_ms = round(sum(rk.values()), 4)
    res["refresh"] = dict(equal=_same_tiling(R, F) and _same_vals_t(torch, ctx, R, F), device_ms=_timed(refresh, ctx, passes, warmup), kernel_ms=r_ms,
                          bytes=int(44 * R.nnz), hbm_frac_kernel=_frac(44 * R.nnz, r_ms))
    for x in [F, R, empty] + distinct + ([A] if all(A is not blk for blk in distinct) else []):
        x.close()
    ctx.close()
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--passes", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--only", default="")
    p.add_argument("--scale", type=float, default=1.0)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "concat_pass.json"))
    a = p.parse_args()
    pkg = g.load_package()
    standins = importlib.import_module("pem_spgemm_amd.standins")
    import torch
    torch.cuda.is_available()
    results = {}
    coo = standins.make("webbase-1M", a.scale)
    for name in a.only.split(",") if a.only else list(DEFAULT):
        r = results[name] = workload(pkg, torch, name, coo, a.passes, a.warmup)
        k, f = r["concat"], r["refresh"]
        print(f"{name}: {r['rows']} x {r['cols']}, {r['cells']} blocks, nnz {r['nnz']}, tiles {r['ntiles']}", flush=True)
        print(f"  {'concat':>10}: equal {r['equal']}, {k['device_ms']:.3f} ms (cc_ kernels {k['concat_kernels_ms']:.3f} ms, all kernels {k['all_kernels_ms']:.3f} ms; "
              f"fill {k['fill_kernel_ms']:.3f} ms, {k['hbm_frac_fill']:.2f} of 8 TB/s)", flush=True)
        print(f"  {'torch':>10}: torch.cat + from_coo_device {r['torch_route_ms']:.3f} ms: {r['ratio_torch']}x", flush=True)
        print(f"  {'assign':>10}: equal {r['assign_equal']}, {r['cells']} assigns {r['assign_route_ms']:.3f} ms: {r['ratio_assign']}x", flush=True)
        print(f"  {'refresh':>10}: equal {f['equal']}, {f['device_ms']:.4f} ms (kernel {f['kernel_ms']:.4f} ms, {f['hbm_frac_kernel']:.2f} of 8 TB/s)", flush=True)
        print("  kernels: " + ", ".join(f"{n} {ms:.3f}" for n, ms in sorted(r["kernels_ms"].items(), key=lambda x: -x[1])[:8]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
