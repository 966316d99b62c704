"""Matrix-vector products and reductions on the device (pem_tiled_mxv / pem_tiled_reduce) against the plan route and rocSPARSE.

    python tools/mxv_pass.py [--passes 10] [--warmup 2] [--only webbase-1M-r2,...] [--out result.json]

Per workload (seeded stand-ins: the numpy webbase-1M stand-in A, its A^2 as a tiling by pem_tiled_from_cplan, cage15 A; each in fp64
and fp32), before any timing: A.x and A^T.x under all six semirings are compared bit for bit with the plan route (A*X resp. X^T*A,
scattered into a dense vector with the start value at empty rows; zero signs under min/max excepted), and reduce(plus) / reduce(max)
over rows and columns with tests/mxvref.py's fold of the exported matrix.  Then, medians over --passes:
  the call's host clock (launch to a context synchronise) and its kernel's device time (the library's per-kernel events), for A.x and
  A^T.x under each semiring and reduce(plus) over rows and columns;
  (a) the plan route as a caller would run it today -- X from the host vector, a plan, steps 1-3 and the CSR export -- and the warm
      repeat pass of that plan alone (steps 1-3, no export);
  (b) torch's CSR tensor @ dense vector on the same CSR (rocSPARSE SpMV), fp64 and fp32, as a reference point.
Bytes: the compulsory traffic of one call -- every entry's 1-byte (r << 4) | c and its value, 8 (rows) or 12 (columns) bytes per tile,
the line pointers, x read once and y written once (no x for a reduction, no values and no x for plus_pair) -- as a fraction of 8 TB/s
over the kernel's device time.
Chain: a 16 x 2^18 matrix whose first row holds every column is one serial chain of 2^18 steps; its kernel time per entry is the cost
of a long row, and the longest row (column) of each workload times that cost is printed next to the kernel time.
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
import mxvref as mr  # noqa: E402

DEFAULT = ("webbase-1M-r2", "webbase-1M-r2^2", "cage15")
SEMIRINGS = mr.SEMIRINGS
MINMAX = ("min_plus", "max_plus", "max_times", "max")


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
    """median device time of the call's kernels (the library's per-kernel events), per call"""
    ts = []
    for _ in range(passes):
        ctx.reset_kernel_stats()
        ctx.set_kernel_profiling(True)
        fn()
        ctx.synchronize()
        ctx.set_kernel_profiling(False)
        ts.append(sum(v["total_ms"] for v in ctx.kernel_stats().values()))
    return statistics.median(ts)


def _bytes(M, col, vb, semiring=None, reduce=False):
    lines = M.tile_cols if col else M.tile_rows
    nx, ny = (M.rows, M.cols) if col else (M.cols, M.rows)
    per_entry = 1 + (0 if semiring == "plus_pair" else vb)
    b = M.nnz * per_entry + M.ntiles * (12 if col else 8) + 4 * (lines + 1) + vb * ny
    if not reduce and semiring != "plus_pair":
        b += vb * nx
    return int(b)


def _frac(nbytes, ms):
    return round(nbytes / (ms * 1e-3) / 8.0e12, 4) if ms > 0 else 0.0


def _same(got, want, kind):
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    ok = (got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want))
    if kind in MINMAX:
        ok |= (got == 0) & (want == 0)
    return bool(np.all(ok))


def _plan_route(pkg, ctx, M, x, semiring, col, export=True):
    n = len(x)
    if col:
        X = pkg.Tiled.from_coo(ctx, 1, n, np.zeros(n, np.int32), np.arange(n, dtype=np.int32), x, dtype=M.dtype)
        p = pkg.CPlan(ctx, X, M, semiring=semiring)
    else:
        X = pkg.Tiled.from_coo(ctx, n, 1, np.arange(n, dtype=np.int32), np.zeros(n, np.int32), x, dtype=M.dtype)
        p = pkg.CPlan(ctx, M, X, semiring=semiring)
    p.spgemm()
    if not export:
        return p, X
    rp, ci, v = p.export_csr()
    y = np.full(M.cols if col else M.rows, mr.MXV_START[semiring], M.dtype)
    if col:
        y[ci] = v
    else:
        y[np.diff(rp) > 0] = v
    p.close()
    X.close()
    return y


def chain_cost(pkg, torch, ctx, passes):
    """kernel time per entry of one serial chain (a 16 x 2^18 matrix, row 0 full), fp64 and fp32"""
    n = 1 << 18
    out = {}
    for dt in (np.float64, np.float32):
        I = np.zeros(n, np.int32)
        J = np.arange(n, dtype=np.int32)
        V = np.random.default_rng(2).standard_normal(n)
        M = pkg.Tiled.from_coo(ctx, 16, n, I, J, V, dtype=dt)
        x = torch.from_numpy(np.random.default_rng(3).standard_normal(n).astype(dt)).cuda()
        y = torch.empty(16, dtype=x.dtype, device="cuda")
        M.mxv(x, out=y)
        ms = _kernel_ms(ctx, lambda: M.mxv(x, out=y), passes)
        out[np.dtype(dt).name] = dict(entries=n, kernel_ms=round(ms, 4), ns_per_entry=round(ms * 1e6 / n, 3))
        M.close()
    return out


def one_matrix(pkg, torch, ctx, M, passes, warmup, ns_per_entry):
    vb = M.value_bytes
    dt = M.dtype
    tdt = getattr(torch, dt.name)
    rp, ci, v = M.export_csr()
    row_len = np.diff(rp)
    col_len = np.bincount(ci, minlength=M.cols)
    r = dict(rows=M.rows, cols=M.cols, nnz=M.nnz, ntiles=M.ntiles, dtype=dt.name, longest_row=int(row_len.max()), longest_col=int(col_len.max()))
    rng = np.random.default_rng(5)
    xs = {False: rng.standard_normal(M.cols).astype(dt), True: rng.standard_normal(M.rows).astype(dt)}
    dx = {k: torch.from_numpy(x).cuda() for k, x in xs.items()}
    ys = {False: torch.empty(M.rows, dtype=tdt, device="cuda"), True: torch.empty(M.cols, dtype=tdt, device="cuda")}
    # checks first
    equal = {}
    for col in (False, True):
        for s in SEMIRINGS:
            M.mxv(dx[col], s, transpose=col, out=ys[col])
            torch.cuda.synchronize()
            equal[f"{s}_{'cols' if col else 'rows'}"] = _same(ys[col].cpu().numpy(), _plan_route(pkg, ctx, M, xs[col], s, col), s)
        dim = "cols" if col else "rows"
        for op in ("plus", "max"):
            M.reduce(op, dim, out=ys[col])
            torch.cuda.synchronize()
            equal[f"reduce_{op}_{dim}"] = _same(ys[col].cpu().numpy(), mr.reduce(M.rows, M.cols, rp, ci, v, op, dt, dim=dim), op)
    r["equal"] = equal
    r["all_equal"] = all(equal.values())
    # timings
    calls = {}
    for col in (False, True):
        o = "cols" if col else "rows"
        for s in SEMIRINGS:
            f = (lambda s=s, col=col: M.mxv(dx[col], s, transpose=col, out=ys[col]))
            k = _kernel_ms(ctx, f, passes)
            nb = _bytes(M, col, vb, semiring=s)
            calls[f"mxv_{s}_{o}"] = dict(wall_ms=round(_median(f, ctx, passes, warmup), 4), kernel_ms=round(k, 4), bytes=nb, hbm_frac=_frac(nb, k))
        f = (lambda col=col: M.reduce("plus", "cols" if col else "rows", out=ys[col]))
        k = _kernel_ms(ctx, f, passes)
        nb = _bytes(M, col, vb, reduce=True)
        calls[f"reduce_plus_{o}"] = dict(wall_ms=round(_median(f, ctx, passes, warmup), 4), kernel_ms=round(k, 4), bytes=nb, hbm_frac=_frac(nb, k))
    r["calls"] = calls
    r["longest_row_chain_ms_est"] = round(r["longest_row"] * ns_per_entry * 1e-6, 4)
    r["longest_col_chain_ms_est"] = round(r["longest_col"] * ns_per_entry * 1e-6, 4)
    # (a) the plan route
    plan_ms = {}
    for col in (False, True):
        o = "cols" if col else "rows"
        plan_ms[f"full_{o}"] = round(_median(lambda col=col: _plan_route(pkg, ctx, M, xs[col], "plus_times", col), ctx, max(1, passes // 5), 1), 3)
        p, X = _plan_route(pkg, ctx, M, xs[col], "plus_times", col, export=False)
        plan_ms[f"warm_pass_{o}"] = round(_median(p.spgemm, ctx, passes, warmup), 4)
        p.close()
        X.close()
    r["plan_route_ms"] = plan_ms
    # (b) rocSPARSE through torch's CSR tensor
    try:
        A = torch.sparse_csr_tensor(torch.from_numpy(rp.astype(np.int64)), torch.from_numpy(ci.astype(np.int64)), torch.from_numpy(v),
                                    size=(M.rows, M.cols)).cuda()
        xv = dx[False].view(-1, 1)
        yv = A @ xv
        torch.cuda.synchronize()
        ts = []
        for i in range(warmup + passes):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            A @ xv
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev = []
        for i in range(passes):
            e0.record()
            A @ xv
            e1.record()
            e1.synchronize()
            ev.append(e0.elapsed_time(e1))
        M.mxv(dx[False], "plus_times", out=ys[False])
        torch.cuda.synchronize()
        rel = float(((yv.view(-1) - ys[False]).abs().max() / ys[False].abs().max().clamp_min(1e-300)).item())
        r["torch_csr_spmv"] = dict(wall_ms=round(statistics.median(ts[warmup:]), 4), event_ms=round(statistics.median(ev), 4),
                                   max_rel_diff_vs_mxv=rel)
        del A
    except Exception as e:   # (not every torch build runs CSR @ dense on the device)
        r["torch_csr_spmv"] = dict(error=f"{type(e).__name__}: {e}")
    return r


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
    stream = torch.cuda.Stream()   # (torch's default stream is the null stream: the context and torch share this one instead)
    torch.cuda.set_stream(stream)
    ctx = pkg.Context(0, stream=stream.cuda_stream)
    results = {"chain": chain_cost(pkg, torch, ctx, a.passes)}
    print(f"chain: one serial row of 2^18 entries: fp64 {results['chain']['float64']['ns_per_entry']:.3f} ns/entry, "
          f"fp32 {results['chain']['float32']['ns_per_entry']:.3f} ns/entry", flush=True)
    for name in names:
        base = name[:-2] if name.endswith("^2") else name
        rows, cols, I, J, V = standins.make(base, 1.0)
        for dt in (np.float64, np.float32):
            A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=dt)
            M, plan = A, None
            if name.endswith("^2"):
                plan = pkg.CPlan(ctx, A, A)
                plan.spgemm()
                M = pkg.Tiled.from_cplan(plan)
                plan.close()
            key = f"{name} {np.dtype(dt).name}"
            r = one_matrix(pkg, torch, ctx, M, a.passes, a.warmup, results["chain"][np.dtype(dt).name]["ns_per_entry"])
            results[key] = r
            c = r["calls"]
            line = (f"{key:>24} nnz {r['nnz']:>10} tiles {r['ntiles']:>9} longest row {r['longest_row']} col {r['longest_col']} | "
                    f"all equal {r['all_equal']}")
            for k in ("mxv_plus_times_rows", "mxv_plus_times_cols", "mxv_min_plus_rows", "mxv_plus_pair_rows", "reduce_plus_rows", "reduce_plus_cols"):
                line += f" | {k} {c[k]['kernel_ms']:.3f} ms ({c[k]['hbm_frac']:.2f} of 8 TB/s, wall {c[k]['wall_ms']:.3f})"
            line += (f" | longest-chain estimate rows {r['longest_row_chain_ms_est']:.3f} ms cols {r['longest_col_chain_ms_est']:.3f} ms"
                     f" | plan route rows {r['plan_route_ms']['full_rows']:.1f} ms (warm pass {r['plan_route_ms']['warm_pass_rows']:.3f})"
                     f" cols {r['plan_route_ms']['full_cols']:.1f} ms (warm pass {r['plan_route_ms']['warm_pass_cols']:.3f})")
            t = r["torch_csr_spmv"]
            line += (f" | torch CSR @ x {t['event_ms']:.3f} ms (wall {t['wall_ms']:.3f}, max rel diff {t['max_rel_diff_vs_mxv']:.2e})"
                     if "event_ms" in t else f" | torch CSR @ x: {t['error']}")
            print(line, flush=True)
            if M is not A:
                M.close()
            A.close()
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
