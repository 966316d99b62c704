"""Building a tiling from triplets with duplicates on the device (pem_tiled_build_device, pem_tiled_set_values_from_build) against
the routes it stands next to.

    python tools/build_pass.py [--passes 10] [--warmup 2] [--only fe_like,heavy_tail] [--scale 1.0] [--out profiles/build_pass.json]

Workloads (seeded):
  fe_like      the webbase-1M stand-in's entries, every one repeated by a run length drawn with mean 4 (1 .. 7), shuffled: about 12 M
               triplets, the shape of a finite-element assembly
  heavy_tail   the same list plus one position hit 1 000 000 times
  mid_runs     90 000 of the stand-in's entries, every one repeated 33 .. 256 times (uniform), shuffled: about 13 M triplets whose
               every run lies where the thresholds 32, 64 and 256 choose different paths (count matrices)
Measured with device events around work that ends in a synchronise, after warm-up, the routes ALTERNATING inside every pass of one
process (medians over --passes):
  (a) build_device against from_coo_device on the already-folded triplets -- the cost of the same output without duplicates; the
      difference is the price of the fold;
  (b) build_device against what a user has today for plus: torch.sparse_coo_tensor(...).coalesce() followed by from_coo_device
      (on a context that shares torch's stream);
  (c) set_values_from_build against a fresh build.
mid_runs and heavy_tail are also built with the long-run path's threshold (PEM_BUILD_INORDER in the environment; never below
PEM_BUILD_INORDER_MAX) at 32, 64 and 256.  Only mid_runs can tell the three apart: heavy_tail has no run of 33 .. 256 values, so
its three figures are the same path measured three times (they bound the noise).
Bytes model, a floor for the WHOLE route: every sort pass reads and writes 12 B per triplet (8 B key, 4 B permutation); the gather
and the fold read 4 B + value_bytes per triplet and the fold writes value_bytes per entry.  "share of the HBM bound" is that floor at
8 TB/s over the measured build time -- a whole-route figure, not a kernel's.
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

DEFAULT = ("fe_like", "heavy_tail", "mid_runs")
ARRAYS = ("tile_keys", "tile_nnz_ptr", "masks", "rowptr", "rowcolidx", "vals", "masks_t", "tile_rowptr", "tile_colidx", "tile_colptr",
          "tile_rowidx", "tile_offsets")


def _bits_for(count):
    b = 0
    while (1 << b) < count:
        b += 1
    return max(b, 1)


def floor_bytes(rows, cols, nnz_in, nnz, value_bytes=8):
    key_bits = 8 + _bits_for((rows + 15) // 16) + _bits_for((cols + 15) // 16)
    passes = (key_bits + 7) // 8
    return passes * 2 * 12 * nnz_in + (4 + value_bytes) * nnz_in + value_bytes * nnz, passes


def _alternating(torch, routes, passes, warmup):
    """{name: median device ms}: the routes one after the other inside every pass"""
    ts = {k: [] for k in routes}
    for i in range(warmup + passes):
        for name, fn in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= warmup:
                ts[name].append(e0.elapsed_time(e1))
            if hasattr(out, "close"):
                out.close()
    return {k: round(statistics.median(v), 4) for k, v in ts.items()}


def _same_tiling(x, y, exact_vals=True):
    for k in ARRAYS:
        a, b = x.array(k), y.array(k)
        if k == "vals" and not exact_vals:
            if not np.allclose(a, b, rtol=1e-9, atol=1e-9):
                return False
        elif not np.array_equal(a.view(np.uint64) if a.dtype.kind == "f" else a, b.view(np.uint64) if b.dtype.kind == "f" else b):
            return False
    return x.nnz == y.nnz and x.ntiles == y.ntiles


def _triplets(standins, name, scale):
    rows, cols, I, J, V = standins.make("webbase-1M", scale)
    rng = np.random.default_rng(2)
    if name == "mid_runs":
        keep = rng.choice(len(I), size=min(len(I), max(1, int(90_000 * scale))), replace=False)
        rep = np.repeat(keep, rng.integers(33, 257, len(keep)))
    else:
        rep = np.repeat(np.arange(len(I)), rng.integers(1, 8, len(I)))      # mean 4
    tI, tJ = I[rep], J[rep]
    if name == "heavy_tail":
        hub = int(rng.integers(0, len(I)))
        tI, tJ = np.concatenate([tI, np.full(1_000_000, I[hub])]), np.concatenate([tJ, np.full(1_000_000, J[hub])])
    p = rng.permutation(len(tI))
    return rows, cols, tI[p].astype(np.int32), tJ[p].astype(np.int32), rng.normal(size=len(p))


def workload(pkg, torch, standins, name, passes, warmup, scale):
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = pkg.Context(0, stream=stream.cuda_stream)
    rows, cols, I, J, V = _triplets(standins, name, scale)
    n_in = len(I)
    dI, dJ, dV = (torch.from_numpy(x).cuda() for x in (I, J, V))
    dIJ = torch.stack([dI.to(torch.int64), dJ.to(torch.int64)])
    torch.cuda.synchronize()
    build = lambda: pkg.Tiled.build_device(ctx, rows, cols, n_in, dI.data_ptr(), dJ.data_ptr(), dV.data_ptr(), dup="plus")
    T = build()
    rp, ci, v = T.export_csr()
    fI = torch.from_numpy(np.repeat(np.arange(rows, dtype=np.int32), np.diff(rp))).cuda()
    fJ, fV = torch.from_numpy(ci).cuda(), torch.from_numpy(v).cuda()
    torch.cuda.synchronize()
    folded = lambda: pkg.Tiled.from_coo_device(ctx, rows, cols, T.nnz, fI.data_ptr(), fJ.data_ptr(), fV.data_ptr())

    def torch_route():
        S = torch.sparse_coo_tensor(dIJ, dV, (rows, cols)).coalesce()
        idx = S.indices().to(torch.int32).contiguous()
        val = S.values()
        out = pkg.Tiled.from_coo_device(ctx, rows, cols, val.numel(), idx[0].data_ptr(), idx[1].data_ptr(), val.data_ptr())
        return out

    nbytes, sort_passes = floor_bytes(rows, cols, n_in, T.nnz)
    res = dict(rows=rows, cols=cols, nnz_in=n_in, nnz=T.nnz, ntiles=T.ntiles, sort_passes=sort_passes, floor_bytes=int(nbytes))
    W = torch_route()
    res["equal_structure_and_close_values_vs_torch"] = _same_tiling(T, W, exact_vals=False)
    W.close()
    ms = _alternating(torch, dict(build=build, from_coo_of_folded=folded, torch_coalesce_then_from_coo=torch_route), passes, warmup)
    res["ms"] = ms
    res["fold_price_ms"] = round(ms["build"] - ms["from_coo_of_folded"], 4)
    res["torch_over_build"] = round(ms["torch_coalesce_then_from_coo"] / ms["build"], 2)
    res["share_of_hbm_bound_whole_route"] = round(nbytes / (ms["build"] * 1e-3) / 8.0e12, 4)
    # (c) refresh against a fresh build
    K = pkg.Tiled.build_device(ctx, rows, cols, n_in, dI.data_ptr(), dJ.data_ptr(), dV.data_ptr(), dup="plus", keep_map=True)
    dV2 = torch.from_numpy(np.random.default_rng(3).normal(size=n_in)).cuda()
    torch.cuda.synchronize()
    K.set_values_from_build(dV2)
    ctx.synchronize()
    F = pkg.Tiled.build_device(ctx, rows, cols, n_in, dI.data_ptr(), dJ.data_ptr(), dV2.data_ptr(), dup="plus")
    res["refresh_equals_fresh_build"] = _same_tiling(K, F)
    F.close()
    fresh2 = lambda: pkg.Tiled.build_device(ctx, rows, cols, n_in, dI.data_ptr(), dJ.data_ptr(), dV2.data_ptr(), dup="plus")
    res["refresh_ms"] = _alternating(torch, dict(refresh=lambda: K.set_values_from_build(dV2), fresh_build=fresh2), passes, warmup)
    if name in ("heavy_tail", "mid_runs"):
        def at(th):
            def run():
                os.environ["PEM_BUILD_INORDER"] = str(th)
                try:
                    return build()
                finally:
                    del os.environ["PEM_BUILD_INORDER"]
            return run
        res["threshold_ms"] = _alternating(torch, {str(th): at(th) for th in (32, 64, 256)}, passes, warmup)
    for x in (K, T):
        x.close()
    ctx.close()
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--passes", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--only", default="")
    p.add_argument("--scale", type=float, default=1.0)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "build_pass.json"))
    a = p.parse_args()
    pkg = g.load_package()
    standins = importlib.import_module("pem_spgemm_amd.standins")
    import torch
    torch.cuda.is_available()
    results = {}
    for name in a.only.split(",") if a.only else list(DEFAULT):
        r = results[name] = workload(pkg, torch, standins, name, a.passes, a.warmup, a.scale)
        m = r["ms"]
        print(f"{name}: {r['rows']} x {r['cols']}, {r['nnz_in']} triplets -> {r['nnz']} entries in {r['ntiles']} tiles, {r['sort_passes']} sort passes", flush=True)
        print(f"  (a) build {m['build']:.3f} ms vs from_coo of the folded entries {m['from_coo_of_folded']:.3f} ms: the fold costs {r['fold_price_ms']:.3f} ms; "
              f"{r['share_of_hbm_bound_whole_route']:.3f} of the HBM bound (whole route)", flush=True)
        print(f"  (b) torch coalesce + from_coo {m['torch_coalesce_then_from_coo']:.3f} ms: {r['torch_over_build']}x the build "
              f"(same structure, close values: {r['equal_structure_and_close_values_vs_torch']})", flush=True)
        print(f"  (c) refresh {r['refresh_ms']['refresh']:.3f} ms vs a fresh build {r['refresh_ms']['fresh_build']:.3f} ms "
              f"(equal: {r['refresh_equals_fresh_build']})", flush=True)
        if "threshold_ms" in r:
            print("  threshold: " + ", ".join(f"{k}: {v:.3f} ms" for k, v in r["threshold_ms"].items()), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
