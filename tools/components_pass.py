"""Connected components on the device (pem_tiled_components) against the routes it replaces.

    python tools/components_pass.py [--passes 7] [--warmup 2] [--scale 1.0] [--cage-scale 1.0] [--grid 1024] [--path 262144]
                                    [--out profiles/components_pass.json]

The graphs, all in fp64 (values are never read) and as stored, symmetric=False (row and column walk):
  webbase-1M, scircuit, cage15   the seeded stand-ins' patterns
  grid       a --grid x --grid 2-D grid on shuffled vertex numbers, every edge stored one way
  path       a path of --path vertices through a shuffled permutation, every edge stored one way
Per graph, warm, in one process: the median of --passes host clocks around A.components() (the call waits by itself), its
components, rounds and time per round, the time inside the round kernels (event pairs around every launch, a run of its own) and,
for scale, one mxv of each orientation -- a round reads every entry's position once per orientation, as the two mxv do, but no
value.  Alongside, on the same tiling in the same run:
  host       A.export_csr() plus scipy.sparse.csgraph.connected_components(directed=False): what a caller does today; the labels
             must agree with the device's
  bfs        where the graph has at most 8 components: one A.bfs per component on the pattern united with its transpose (bfs
             follows stored directions), the next source found on the host -- one wait per level.  One pass: a path's levels are
             its vertices.
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as g  # noqa: E402
from trsv_pass import _median  # noqa: E402


def _stats(t):
    med, lo, hi = t
    return dict(median=round(med, 4), min=round(lo, 4), max=round(hi, 4))


def grid_graph(side, seed=64):
    q = np.random.default_rng(seed).permutation(side * side).reshape(side, side)
    I = np.concatenate([q[:, :-1].ravel(), q[:-1, :].ravel()])
    J = np.concatenate([q[:, 1:].ravel(), q[1:, :].ravel()])
    return side * side, I.astype(np.int32), J.astype(np.int32)


def path_graph(n, seed=5000):
    q = np.random.default_rng(seed).permutation(n)
    return n, q[:-1].astype(np.int32), q[1:].astype(np.int32)


def symmetrised(n, I, J):
    I, J = np.asarray(I, np.int64), np.asarray(J, np.int64)
    key = np.unique(np.concatenate([I * n + J, J * n + I]))
    return (key // n).astype(np.int32), (key % n).astype(np.int32)


def host_route(A):
    """(seconds, labels): export_csr, then scipy's components mapped to smallest-vertex labels"""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    n = A.rows
    t0 = time.perf_counter()
    rp, ci, v = A.export_csr()
    t1 = time.perf_counter()
    M = sp.csr_matrix((np.ones(len(ci), np.int8), ci, rp), shape=(n, n))
    nc, lab = connected_components(M, directed=False)
    t2 = time.perf_counter()
    smallest = np.full(nc, n, np.int64)
    np.minimum.at(smallest, lab, np.arange(n))
    return dict(export_seconds=round(t1 - t0, 4), scipy_seconds=round(t2 - t1, 4), seconds=round(t2 - t0, 4), components=int(nc)), \
        smallest[lab].astype(np.int32)


def bfs_route(torch, ctx, S):
    """one bfs per component on the symmetric tiling S; the next source is the first vertex no search has reached"""
    n = S.rows
    t0 = time.perf_counter()
    label = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    src, searches, levels = 0, 0, 0
    while src < n:
        lv, depth, _ = S.bfs(src)
        label = torch.where((lv >= 0) & (label < 0), torch.full_like(label, src), label)
        searches, levels = searches + 1, levels + depth
        rest = torch.nonzero(label < 0)
        src = int(rest[0]) if rest.numel() else n
    ctx.synchronize()
    torch.cuda.synchronize()
    return dict(seconds=round(time.perf_counter() - t0, 4), searches=searches, levels=levels), label


def measure(pkg, torch, ctx, name, n, I, J, passes, warmup):
    A = pkg.Tiled.from_coo(ctx, n, n, I, J, np.ones(len(I)))
    r = dict(n=n, nnz=len(I))
    labels, ids, nc, rounds = A.components()
    t = _stats(_median(lambda: A.components(out=labels, out_ids=ids), ctx, passes, warmup))
    r.update(components=nc, rounds=rounds, components_ms=t, us_per_round=round(1e3 * t["median"] / max(1, rounds), 3))
    t = _stats(_median(lambda: A.components(out=labels, ids=False), ctx, passes, warmup))
    r["components_no_ids_ms"] = t
    # the rounds' kernels alone (event pairs around every launch): what the call spends outside them is launches and read-backs
    ctx.reset_kernel_stats()
    ctx.set_kernel_profiling(True)
    A.components(out=labels, out_ids=ids)
    ctx.synchronize()
    ks = ctx.kernel_stats()
    ctx.set_kernel_profiling(False)
    r["kernels_ms"] = {k: round(v["total_ms"], 4) for k, v in ks.items() if k.startswith("components_")}
    x = torch.from_numpy(np.random.default_rng(3).standard_normal(n)).cuda()
    y = torch.empty_like(x)
    A.mxv(x, out=y), A.mxv(x, transpose=True, out=y)
    r["mxv_ms"] = _stats(_median(lambda: A.mxv(x, out=y), ctx, passes, warmup))
    r["mxv_transpose_ms"] = _stats(_median(lambda: A.mxv(x, transpose=True, out=y), ctx, passes, warmup))
    torch.cuda.synchronize()
    dev = labels.cpu().numpy()
    r["host"], want = host_route(A)
    r["host"]["equals_device"] = bool(np.array_equal(dev, want)) and r["host"]["components"] == nc
    r["host_over_device"] = round(1e3 * r["host"]["seconds"] / r["components_ms"]["median"], 1)
    line = (f"{name:>10}: n {n} nnz {len(I)} | {nc} components in {rounds} rounds | components {r['components_ms']['median']:.3f} ms "
            f"({r['us_per_round']:.1f} us/round; without ids {r['components_no_ids_ms']['median']:.3f} ms; kernels "
            f"{sum(r['kernels_ms'].values()):.3f} ms) | mxv {r['mxv_ms']['median']:.3f} + {r['mxv_transpose_ms']['median']:.3f} ms | host "
            f"{r['host']['seconds']:.3f} s (export {r['host']['export_seconds']:.3f} s), same labels {r['host']['equals_device']}")
    if nc <= 8:
        Is, Js = symmetrised(n, I, J)
        S = pkg.Tiled.from_coo(ctx, n, n, Is, Js, np.ones(len(Is)))
        S.bfs(0)
        r["bfs"], bl = bfs_route(torch, ctx, S)
        r["bfs"]["equals_device"] = bool(torch.equal(bl, labels))
        r["bfs_over_device"] = round(1e3 * r["bfs"]["seconds"] / r["components_ms"]["median"], 1)
        line += f" | bfs route {r['bfs']['seconds']:.3f} s ({r['bfs']['searches']} searches, {r['bfs']['levels']} levels), same labels {r['bfs']['equals_device']}"
        S.close()
    print(line, flush=True)
    A.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--cage-scale", type=float, default=1.0)
    ap.add_argument("--grid", type=int, default=1024)
    ap.add_argument("--path", type=int, default=262144)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pkg = g.load_package()
    standins = importlib.import_module("pem_spgemm_amd.standins")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("components_pass: no GPU (this tool measures on the device only)")
    stream = torch.cuda.Stream()   # (torch's default stream is the null stream: the context and torch share this one instead)
    torch.cuda.set_stream(stream)
    ctx = pkg.Context(0, stream=stream.cuda_stream)

    def standin(name, scale):
        rows, cols, I, J, _ = standins.make(name, scale)
        return max(rows, cols), I, J

    graphs = {"webbase-1M": lambda: standin("webbase-1M", a.scale), "scircuit": lambda: standin("scircuit", a.scale),
              "cage15": lambda: standin("cage15", a.cage_scale), "grid": lambda: grid_graph(a.grid), "path": lambda: path_graph(a.path)}
    results = dict(passes=a.passes, warmup=a.warmup, scale=a.scale, cage_scale=a.cage_scale, grid=a.grid, path=a.path, graphs={})
    for name, make in graphs.items():
        if a.only and name not in a.only.split(","):
            continue
        n, I, J = make()
        results["graphs"][name] = measure(pkg, torch, ctx, name, n, I, J, a.passes, a.warmup)
        if a.out:   # (after every graph: a run that is cut short keeps what it measured)
            with open(a.out, "w") as f:
                json.dump(results, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
