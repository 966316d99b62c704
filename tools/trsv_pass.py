"""Triangular solve on the device (pem_tiled_trsv) on three orderings of one problem, against its floor and against torch.

    python tools/trsv_pass.py [--passes 7] [--warmup 2] [--scale 1.0] [--out profiles/trsv_pass.json]

The matrix: the seeded webbase-1M stand-in's off-diagonal pattern, symmetrised, with standard normal values and a dominant diagonal
(+-(row abs sum + 1 + U[0, 1)), so every solve stays finite); the solve is on its LOWER triangle, the full matrix handed over as it
is (the other side is ignored).  Three matrices of the same n, fp64:
  natural    the stand-in's own numbering
  coloured   the same matrix after a greedy colouring (natural order, smallest free colour), the vertices sorted by colour,
             reordered on the device by extract(p, p): inside a colour no vertex waits for another
  bidiagonal the worst case of the same n: every tile row waits for the one before
Per matrix: levels, launches and the widest level (pem_tiled_trsv_info); the one-off schedule time (the first call's host clock, a
synchronise at its end); then, warm and with the schedule cached, medians over --passes of the host clock around one solve that
ends in a context synchronise -- with the narrow levels merged, and with merging forced off (one launch per level).  Both routes
must give the same bits, and the solve's residual against the library's own mxv on the triangle is printed.  Alongside: one mxv on
the same triangle (select("tril", 0)) -- the same bytes, no dependencies: the floor -- and torch's sparse-CSR triangular solve on
the device where this torch build has one ("absent" otherwise).
Bytes: every entry of the triangle (1-byte position + value), 8 bytes per tile, 24 per tile row, b read and x written once, as a
fraction of 8 TB/s over the solve's time (a whole-call rate: launches and barriers included).
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


def _median(fn, ctx, passes, warmup):
    ts = [_wall(fn, ctx) for _ in range(warmup + passes)]
    return statistics.median(ts[warmup:]), min(ts[warmup:]), max(ts[warmup:])


def symmetric_problem(standins, scale, seed=7):
    """(n, I, J, V): the stand-in's off-diagonal pattern on both sides, normal values, a dominant diagonal"""
    rows, cols, I, J, _ = standins.make("webbase-1M", scale)
    n = max(rows, cols)
    I, J = np.asarray(I, np.int64), np.asarray(J, np.int64)
    off = I != J
    lo, hi = np.minimum(I[off], J[off]), np.maximum(I[off], J[off])
    key = np.unique(hi * n + lo)
    hi, lo = key // n, key % n
    return with_diagonal(n, np.concatenate([hi, lo]), np.concatenate([lo, hi]), np.random.default_rng(seed))


def with_diagonal(n, I, J, rng):
    V = rng.standard_normal(len(I))
    s = np.zeros(n)
    np.add.at(s, I, np.abs(V))
    d = (s + 1.0 + rng.random(n)) * rng.choice([-1.0, 1.0], n)
    ar = np.arange(n, dtype=np.int64)
    return n, np.concatenate([I, ar]).astype(np.int32), np.concatenate([J, ar]).astype(np.int32), np.concatenate([V, d])


def greedy_colouring(n, I, J):
    """colour[v]: the smallest colour no neighbour with a smaller number holds (vertices in natural order)"""
    o = np.lexsort((J, I))
    ci = J[o].tolist()
    rp = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(I, minlength=n), out=rp[1:])
    rp = rp.tolist()
    colour = [0] * n
    for v in range(n):
        used = {colour[u] for u in ci[rp[v]:rp[v + 1]] if u < v}
        c = 0
        while c in used:
            c += 1
        colour[v] = c
    return np.array(colour, np.int64)


def measure(pkg, torch, ctx, S, label, passes, warmup):
    n, vb = S.rows, S.value_bytes
    tdt = getattr(torch, S.dtype.name)
    b = torch.from_numpy(np.random.default_rng(11).standard_normal(n)).cuda().to(tdt)
    x = torch.empty_like(b)
    r = dict(n=n, nnz_full=S.nnz, dtype=S.dtype.name)
    ctx.trsv_split(False)
    r["schedule_ms"] = round(_wall(lambda: S.trsv_info("lower"), ctx), 3)
    info = S.trsv_info("lower")
    r.update(levels=info["levels"], launches=info["launches"], max_width=info["max_width"], merge_width=info["merge_width"])
    T = S.select("tril", 0)
    r.update(nnz_triangle=T.nnz, ntiles_triangle=T.ntiles)
    nbytes = T.nnz * (1 + vb) + 8 * T.ntiles + 24 * T.tile_rows + 2 * vb * n
    r["bytes"] = int(nbytes)
    S.trsv(b, "lower", out=x)
    med, lo, hi = _median(lambda: S.trsv(b, "lower", out=x), ctx, passes, warmup)
    r["solve_ms"] = dict(median=round(med, 4), min=round(lo, 4), max=round(hi, 4), hbm_frac=round(nbytes / (med * 1e-3) / 8.0e12, 5))
    merged_bits = x.clone()
    # the residual, by the library's own mxv on the triangle
    t = T.mxv(x)
    ctx.synchronize()
    torch.cuda.synchronize()
    r["residual_inf_rel"] = float(((t - b).abs().max() / b.abs().max()).item())
    ctx.trsv_split(True)
    r["launches_split"] = S.trsv_info("lower")["launches"]
    S.trsv(b, "lower", out=x)
    slow = r["launches_split"] > 20000
    med, lo, hi = _median(lambda: S.trsv(b, "lower", out=x), ctx, max(3, passes // 2) if slow else passes, 1 if slow else warmup)
    r["solve_split_ms"] = dict(median=round(med, 4), min=round(lo, 4), max=round(hi, 4))
    ctx.synchronize()
    torch.cuda.synchronize()
    r["split_equals_merged"] = bool(torch.equal(x.view(torch.int64 if vb == 8 else torch.int32), merged_bits.view(torch.int64 if vb == 8 else torch.int32)))
    ctx.trsv_split(False)
    # the floor: one mxv on the same triangle
    y = torch.empty_like(b)
    T.mxv(b, out=y)
    med, lo, hi = _median(lambda: T.mxv(b, out=y), ctx, passes, warmup)
    r["mxv_triangle_ms"] = dict(median=round(med, 4), min=round(lo, 4), max=round(hi, 4))
    # torch's sparse-CSR triangular solve on the device, where this build has one
    try:
        rp, ci, v = T.export_csr()
        A = torch.sparse_csr_tensor(torch.from_numpy(rp.astype(np.int64)), torch.from_numpy(ci.astype(np.int64)), torch.from_numpy(v),
                                    size=(n, n)).cuda()
        bb = b.view(-1, 1)
        xs = torch.triangular_solve(bb, A, upper=False).solution
        torch.cuda.synchronize()
        ts = []
        for _ in range(warmup + passes):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            torch.triangular_solve(bb, A, upper=False)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        rel = float(((xs.view(-1) - merged_bits).abs().max() / merged_bits.abs().max()).item())
        r["torch_csr_triangular_solve"] = dict(median_ms=round(statistics.median(ts[warmup:]), 4), max_rel_diff_vs_trsv=rel)
        del A
    except Exception as e:   # (not every torch build solves sparse CSR triangles on the device)
        r["torch_csr_triangular_solve"] = dict(absent=f"{type(e).__name__}: {str(e)[:200]}")
    T.close()
    t = r["torch_csr_triangular_solve"]
    print(f"{label:>10} n {n} triangle nnz {r['nnz_triangle']} | levels {r['levels']} launches {r['launches']} (split {r['launches_split']}) "
          f"max width {r['max_width']} | schedule {r['schedule_ms']:.1f} ms | solve {r['solve_ms']['median']:.3f} ms "
          f"({r['solve_ms']['hbm_frac']:.4f} of 8 TB/s) | merging off {r['solve_split_ms']['median']:.3f} ms, same bits {r['split_equals_merged']} | "
          f"mxv on the triangle {r['mxv_triangle_ms']['median']:.3f} ms | residual {r['residual_inf_rel']:.2e} | torch: "
          + (f"{t['median_ms']:.3f} ms (max rel diff {t['max_rel_diff_vs_trsv']:.1e})" if "median_ms" in t else "absent"), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pkg = g.load_package()
    standins = importlib.import_module("pem_spgemm_amd.standins")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("trsv_pass: no GPU (this tool measures on the device only)")
    stream = torch.cuda.Stream()   # (torch's default stream is the null stream: the context and torch share this one instead)
    torch.cuda.set_stream(stream)
    ctx = pkg.Context(0, stream=stream.cuda_stream)
    n, I, J, V = symmetric_problem(standins, a.scale)
    results = dict(workload=f"webbase-1M stand-in (scale {a.scale}), symmetrised pattern, lower triangle", passes=a.passes, warmup=a.warmup)
    S = pkg.Tiled.from_coo(ctx, n, n, I, J, V)
    results["natural"] = measure(pkg, torch, ctx, S, "natural", a.passes, a.warmup)
    t0 = time.perf_counter()
    colour = greedy_colouring(n, I.astype(np.int64), J.astype(np.int64))
    p = np.argsort(colour, kind="stable").astype(np.int32)
    results["colouring"] = dict(colours=int(colour.max()) + 1, host_seconds=round(time.perf_counter() - t0, 2))
    R = S.extract(p, p)
    S.close()
    results["coloured"] = measure(pkg, torch, ctx, R, "coloured", a.passes, a.warmup)
    R.close()
    i = np.arange(1, n, dtype=np.int64)
    _, bi, bj, bv = with_diagonal(n, i, i - 1, np.random.default_rng(8))
    B = pkg.Tiled.from_coo(ctx, n, n, bi, bj, bv)
    results["bidiagonal"] = measure(pkg, torch, ctx, B, "bidiagonal", a.passes, a.warmup)
    B.close()
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
