"""Arg folds on the device (pem_tiled_mxv_arg / pem_tiled_reduce_arg / pem_tiled_bfs_parents) against the value-only calls of the
same semiring on the same tiling, and against a torch route over the exported CSR.

    python tools/arg_pass.py [--passes 10] [--warmup 2] [--only webbase-1M-r2,powerlaw-hubs] [--out profiles/arg_pass.json]

Per workload (seeded stand-ins, fp64: the webbase-1M stand-in, and `powerlaw-hubs`, a power-law matrix made here whose longest rows
hold tens of thousands of entries -- the long-row path), medians over --passes after --warmup of the call's host clock (launch to a
context synchronise) and of its kernels' device time (the library's per-kernel events), both orientations:
  dense     x all present, no mask, under min_plus, max_plus and max_times: pem_tiled_mxv, pem_tiled_mxv_frontier with x_present =
            None (the walk the arg walk was copied from) and pem_tiled_mxv_arg; the values compared bit for bit (up to zero signs);
            ratio of the arg walk to each.  min_index / max_index against the frontier walk under plus_pair, which loads what they
            load.
  frontier  half of x present and half of the outputs allowed (independent draws): mxv_frontier against mxv_arg, min_plus and
            min_index (against plus_pair).
  reduce    pem_tiled_reduce(min | max) against pem_tiled_reduce_arg.
  bfs       from the highest-degree vertex: pem_tiled_bfs against pem_tiled_bfs_parents (host clock: both wait), levels compared.
  torch     the route without the library's arg fold: export_csr (host clock, once) and then, on the device, per row the max
            by torch.segment_reduce and its first position by a second segment_reduce over the positions where the value equals it.
Bytes: what the dense arg call must move -- per tile its offset, minor index (and base, for columns): 8 or 12 bytes; per entry its
1-byte (major, minor), its value and its x (2 x 8 bytes; the reductions: one); per output the value and the 4-byte index written
-- as a share of 8 TB/s over the kernel time.  The value walk moves the same less the 4 bytes per output.
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

DEFAULT = ("webbase-1M-r2", "powerlaw-hubs")
VALUE_KINDS = ("min_plus", "max_plus", "max_times")


def powerlaw_hubs(seed=11, n=400_000):
    """power-law out-degrees (Pareto, shape 1.1) capped at 60000, uniform columns: a few rows of tens of thousands of entries"""
    rng = np.random.default_rng(seed)
    deg = np.minimum((rng.pareto(1.1, n) + 1).astype(np.int64), 60000)
    I = np.repeat(np.arange(n, dtype=np.int64), deg)
    key = np.unique(I * n + rng.integers(0, n, len(I)))
    return n, n, (key // n).astype(np.int32), (key % n).astype(np.int32), rng.uniform(-1.0, 1.0, len(key))


def _wall(fn, ctx):
    ctx.synchronize()
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _median(fn, ctx, passes, warmup):
    ts = [_wall(fn, ctx) for _ in range(warmup + passes)]
    return statistics.median(ts[warmup:])


def _kernel_ms(ctx, fn, passes):
    ts = []
    for _ in range(passes):
        ctx.reset_kernel_stats()
        ctx.set_kernel_profiling(True)
        fn()
        ctx.synchronize()
        ctx.set_kernel_profiling(False)
        ts.append(sum(v["total_ms"] for v in ctx.kernel_stats().values()))
    return statistics.median(ts)


def _timed(ctx, fn, passes, warmup):
    fn()
    return dict(kernel_ms=round(_kernel_ms(ctx, fn, passes), 4), wall_ms=round(_median(fn, ctx, passes, warmup), 4))


def _ratio(a, b, key="kernel_ms"):
    return round(a[key] / b[key], 3) if b[key] > 0 else 0.0


def _frac(nbytes, ms):
    return round(nbytes / (ms * 1e-3) / 8.0e12, 4) if ms > 0 else 0.0


def _same_values(torch, a, b):
    """equal bits, or both zero (the sign of a zero under min / max is not specified)"""
    return bool((((a.view(torch.int64) == b.view(torch.int64)) | ((a == 0) & (b == 0))).all()))


def torch_route(torch, ctx, M, passes, warmup):
    t0 = time.perf_counter()
    rp, ci, v = M.export_csr()
    r = dict(export_csr_wall_ms=round((time.perf_counter() - t0) * 1e3, 3))
    try:
        drp, dci, dv = (torch.from_numpy(a).cuda() for a in (rp.astype(np.int64), ci.astype(np.int64), v))
        rows = torch.repeat_interleave(torch.arange(M.rows, device="cuda"), drp[1:] - drp[:-1])
        pos = torch.arange(len(v), dtype=torch.float64, device="cuda")

        def route():
            best = torch.segment_reduce(dv, "max", offsets=drp, initial=float("-inf"))
            first = torch.segment_reduce(torch.where(dv == best[rows], pos, float("inf")), "min", offsets=drp, initial=float("inf"))
            has = torch.isfinite(first)
            idx = torch.where(has, dci[first.clamp(0, max(len(v) - 1, 0)).long()], -1)
            return best, idx.int()

        best, idx = route()
        y, gi = M.reduce_arg("max", "rows")
        torch.cuda.synchronize()
        r["equal_to_reduce_arg"] = _same_values(torch, best, y) and bool(torch.equal(idx, gi))
        torch.cuda.synchronize()
        ts = []
        for _ in range(warmup + passes):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            route()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        r["segment_reduce_argmax_wall_ms"] = round(statistics.median(ts[warmup:]), 4)
    except Exception as e:   # (an operator this torch build lacks: reported, not worked around)
        r["unavailable"] = f"{type(e).__name__}: {e}"[:300]
    return r


def one_matrix(pkg, torch, ctx, M, passes, warmup):
    r = dict(rows=M.rows, cols=M.cols, nnz=M.nnz, ntiles=M.ntiles)
    rng = np.random.default_rng(5)
    dense, frontier, reduce_ = {}, {}, {}
    for col in (False, True):
        o = "cols" if col else "rows"
        nx, ny = (M.rows, M.cols) if col else (M.cols, M.rows)
        x = torch.from_numpy(rng.standard_normal(nx)).cuda()
        ya, yb = (torch.empty(ny, dtype=torch.float64, device="cuda") for _ in range(2))
        idx = torch.empty(ny, dtype=torch.int32, device="cuda")
        present, mask = torch.from_numpy(rng.random(nx) < 0.5).cuda(), torch.from_numpy(rng.random(ny) < 0.5).cuda()
        tile_bytes = M.ntiles * (12 if col else 8)
        for kind in VALUE_KINDS:
            a = _timed(ctx, lambda: M.mxv(x, kind, transpose=col, out=ya), passes, warmup)
            f = _timed(ctx, lambda: M.mxv_frontier(x, semiring=kind, transpose=col, out=ya), passes, warmup)
            b = _timed(ctx, lambda: M.mxv_arg(x, kind, col, out=yb, out_index=idx), passes, warmup)
            nb = tile_bytes + M.nnz * 17 + ny * 12
            dense[f"{kind}_{o}"] = dict(mxv=a, frontier=f, arg=b, equal=_same_values(torch, ya, yb), bytes=nb, hbm_frac_arg=_frac(nb, b["kernel_ms"]),
                                        kernel_ratio_to_mxv=_ratio(b, a), kernel_ratio_to_frontier=_ratio(b, f),
                                        wall_ratio_to_mxv=_ratio(b, a, "wall_ms"), wall_ratio_to_frontier=_ratio(b, f, "wall_ms"))
        f = _timed(ctx, lambda: M.mxv_frontier(None, semiring="plus_pair", transpose=col, out=ya), passes, warmup)
        for kind in ("min_index", "max_index"):
            b = _timed(ctx, lambda: M.mxv_arg(None, kind, col, out_index=idx), passes, warmup)
            dense[f"{kind}_{o}"] = dict(frontier_plus_pair=f, arg=b, kernel_ratio_to_frontier=_ratio(b, f), wall_ratio_to_frontier=_ratio(b, f, "wall_ms"))
        f = _timed(ctx, lambda: M.mxv_frontier(x, present, mask, False, "min_plus", col, out=ya), passes, warmup)
        b = _timed(ctx, lambda: M.mxv_arg(x, "min_plus", col, present, mask, False, yb, idx), passes, warmup)
        frontier[f"min_plus_{o}"] = dict(frontier=f, arg=b, kernel_ratio=_ratio(b, f), wall_ratio=_ratio(b, f, "wall_ms"))
        f = _timed(ctx, lambda: M.mxv_frontier(None, present, mask, False, "plus_pair", col, out=ya), passes, warmup)
        b = _timed(ctx, lambda: M.mxv_arg(None, "min_index", col, present, mask, False, None, idx), passes, warmup)
        frontier[f"min_index_{o}"] = dict(frontier_plus_pair=f, arg=b, kernel_ratio=_ratio(b, f), wall_ratio=_ratio(b, f, "wall_ms"))
        for op in ("min", "max"):
            a = _timed(ctx, lambda: M.reduce(op, o, out=ya), passes, warmup)
            b = _timed(ctx, lambda: M.reduce_arg(op, o), passes, warmup)
            y2, _ = M.reduce_arg(op, o)
            nb = tile_bytes + M.nnz * 9 + ny * 12
            reduce_[f"{op}_{o}"] = dict(reduce=a, reduce_arg=b, equal=_same_values(torch, ya, y2), hbm_frac_arg=_frac(nb, b["kernel_ms"]),
                                        kernel_ratio=_ratio(b, a), wall_ratio=_ratio(b, a, "wall_ms"))
    r["dense"], r["frontier"], r["reduce"] = dense, frontier, reduce_
    if M.rows == M.cols:
        rp, _, _ = M.export_csr()
        src = int(np.argmax(np.diff(rp)))
        lv, depth, reached = M.bfs(src)
        lv2, par, depth2, reached2 = M.bfs_parents(src)
        torch.cuda.synchronize()
        b = dict(source=src, depth=depth, reached=reached, equal=bool(torch.equal(lv, lv2)) and (depth, reached) == (depth2, reached2),
                 with_parent=int((par >= 0).sum()))
        b["pem_tiled_bfs_wall_ms"] = round(_median(lambda: M.bfs(src), ctx, passes, warmup), 4)
        b["pem_tiled_bfs_parents_wall_ms"] = round(_median(lambda: M.bfs_parents(src), ctx, passes, warmup), 4)
        b["wall_ratio"] = round(b["pem_tiled_bfs_parents_wall_ms"] / b["pem_tiled_bfs_wall_ms"], 3)
        r["bfs"] = b
    r["torch"] = torch_route(torch, ctx, M, passes, warmup)
    return r


def report(name, r):
    out = [f"{name}: {r['rows']} x {r['cols']}, nnz {r['nnz']}, tiles {r['ntiles']}"]
    out.append("  dense (all present, no mask): kernel ms (wall ms)      mxv | frontier walk | arg walk: ratio to mxv, to the frontier walk")
    for k, d in r["dense"].items():
        if "mxv" in d:
            out.append(f"    {k:>16}  {d['mxv']['kernel_ms']:.4f} ({d['mxv']['wall_ms']:.4f}) | {d['frontier']['kernel_ms']:.4f} ({d['frontier']['wall_ms']:.4f}) | "
                       f"{d['arg']['kernel_ms']:.4f} ({d['arg']['wall_ms']:.4f}) x{d['kernel_ratio_to_mxv']:.3f} x{d['kernel_ratio_to_frontier']:.3f}"
                       f" | values equal {d['equal']} | {d['hbm_frac_arg']:.3f} of 8 TB/s")
        else:
            f = d["frontier_plus_pair"]
            out.append(f"    {k:>16}  plus_pair walk {f['kernel_ms']:.4f} ({f['wall_ms']:.4f}) | {d['arg']['kernel_ms']:.4f} ({d['arg']['wall_ms']:.4f})"
                       f" x{d['kernel_ratio_to_frontier']:.3f}")
    out.append("  half of x present, half of the outputs allowed: kernel ms (wall ms)      value-only | arg")
    for k, d in r["frontier"].items():
        f = d.get("frontier", d.get("frontier_plus_pair"))
        out.append(f"    {k:>16}  {f['kernel_ms']:.4f} ({f['wall_ms']:.4f}) | {d['arg']['kernel_ms']:.4f} ({d['arg']['wall_ms']:.4f}) x{d['kernel_ratio']:.3f}")
    out.append("  reduce | reduce_arg: kernel ms (wall ms)")
    for k, d in r["reduce"].items():
        out.append(f"    {k:>16}  {d['reduce']['kernel_ms']:.4f} ({d['reduce']['wall_ms']:.4f}) | {d['reduce_arg']['kernel_ms']:.4f} ({d['reduce_arg']['wall_ms']:.4f})"
                   f" x{d['kernel_ratio']:.3f} | values equal {d['equal']} | {d['hbm_frac_arg']:.3f} of 8 TB/s")
    if "bfs" in r:
        b = r["bfs"]
        out.append(f"  bfs from {b['source']}: depth {b['depth']}, reached {b['reached']}, levels equal {b['equal']}: pem_tiled_bfs {b['pem_tiled_bfs_wall_ms']:.3f} ms | "
                   f"pem_tiled_bfs_parents {b['pem_tiled_bfs_parents_wall_ms']:.3f} ms x{b['wall_ratio']:.3f}")
    t = r["torch"]
    if "unavailable" in t:
        out.append(f"  torch route: export_csr {t['export_csr_wall_ms']:.1f} ms; segment_reduce route unavailable ({t['unavailable']})")
    else:
        out.append(f"  torch route: export_csr {t['export_csr_wall_ms']:.1f} ms, then segment_reduce argmax of rows {t['segment_reduce_argmax_wall_ms']:.3f} ms"
                   f" (equal to reduce_arg {t['equal_to_reduce_arg']}); reduce_arg max rows {r['reduce']['max_rows']['reduce_arg']['wall_ms']:.3f} ms")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pkg = g.load_package()
    standins = importlib.import_module("pem_spgemm_amd.standins")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("arg_pass: no GPU (this tool measures on the device; there is no fallback)")
    names = a.only.split(",") if a.only else list(DEFAULT)
    stream = torch.cuda.Stream()   # (torch's default stream is the null stream: the context and torch share this one instead)
    torch.cuda.set_stream(stream)
    ctx = pkg.Context(0, stream=stream.cuda_stream)
    results = {"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "passes": a.passes, "warmup": a.warmup}
    for name in names:
        rows, cols, I, J, V = powerlaw_hubs(n=int(400_000 * a.scale)) if name == "powerlaw-hubs" else standins.make(name, a.scale)
        A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
        results[name] = one_matrix(pkg, torch, ctx, A, a.passes, a.warmup)
        print(report(name, results[name]), flush=True)
        A.close()
        if a.out:
            with open(a.out, "w") as f:
                json.dump(results, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
