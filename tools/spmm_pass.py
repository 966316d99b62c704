"""A tiling times a dense block of k vectors on the device (pem_tiled_spmm) against k mxv calls, rocSPARSE and the plan route.
    python tools/spmm_pass.py [--passes 10] [--warmup 2] [--only webbase-1M-r2,...] [--ks 1,4,16,64] [--out result.json]
Per workload (seeded stand-ins: the numpy webbase-1M stand-in A, its A^2 as a tiling by pem_tiled_from_cplan, cage15 A; fp64 and
fp32), before any timing: A.X and A^T.X (k = 5) under all six semirings are compared column by column with pem_tiled_mxv, bit for bit
(zero signs under min/max excepted).  Then, medians over --passes after --warmup, for each k:
  the call's kernel device time (the library's per-kernel events) and host clock (launch to a context synchronise), A.X and A^T.X
  under plus_times, and A.X under min_plus;
  (a) k mxv calls, one per column (kernel time);
  (b) torch's CSR tensor @ dense block on the same CSR (rocSPARSE SpMM), event time;
  (c) for k <= 16, the plan route with X an n x k tiling storing every entry: the warm repeat pass of the plan alone (steps 1-3).
The heaviest line: the tile row with the most entries, cut out by two positional selects, timed alone at k = 1 (the spmm
kernel on a column slice) and k = 4 against mxv.
Bytes: the compulsory traffic -- A once per column block (1 + value bytes per entry, 8 or 12 per tile, the line pointers), X read
once and Y written once -- as a fraction of 8 TB/s over the kernel time; and the gathered bytes nnz * k * value_bytes, which the
caches serve in part, printed apart so that a cache-served rate is not read as an HBM one.
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
MINMAX = ("min_plus", "max_plus", "max_times")


def _widthblocks(k):
    w = 4 if k <= 4 else 8 if k <= 8 else 16
    return (k + w - 1) // w


def _wall(fn, ctx, passes, warmup):
    ts = []
    for _ in range(warmup + passes):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts[warmup:])


def _kernel_ms(ctx, fn, passes, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(passes):
        ctx.reset_kernel_stats()
        ctx.set_kernel_profiling(True)
        fn()
        ctx.synchronize()
        ctx.set_kernel_profiling(False)
        ts.append(sum(v["total_ms"] for v in ctx.kernel_stats().values()))
    return statistics.median(ts)


def _bytes(M, col, vb, k):
    lines = M.tile_cols if col else M.tile_rows
    nx, ny = (M.rows, M.cols) if col else (M.cols, M.rows)
    a = M.nnz * (1 + vb) + M.ntiles * (12 if col else 8) + 4 * (lines + 1)
    return int(a * _widthblocks(k) + vb * k * (nx + ny))


def _frac(nbytes, ms):
    return round(nbytes / (ms * 1e-3) / 8.0e12, 4) if ms > 0 else 0.0


def _same(got, want, kind):
    """bit equality of two device tensors of one shape (NaN == NaN; +0 == -0 under min/max)"""
    import torch
    gb, wb = got.contiguous().view(-1), want.contiguous().view(-1)
    it = torch.int64 if gb.dtype == torch.float64 else torch.int32
    ok = (gb.view(it) == wb.view(it)) | (gb.isnan() & wb.isnan())
    if kind in MINMAX:
        ok |= (gb == 0) & (wb == 0)
    return bool(ok.all().item())


def one_matrix(pkg, torch, ctx, M, ks, passes, warmup):
    vb = M.value_bytes
    tdt = getattr(torch, M.dtype.name)
    r = dict(rows=M.rows, cols=M.cols, nnz=M.nnz, ntiles=M.ntiles, dtype=M.dtype.name)
    rng = np.random.default_rng(5)
    # checks first: column by column against pem_tiled_mxv, every semiring, both orientations
    equal = {}
    kc = 5
    for col in (False, True):
        nx, ny = (M.rows, M.cols) if col else (M.cols, M.rows)
        X = torch.from_numpy(rng.standard_normal((nx, kc)).astype(M.dtype)).cuda()
        for s in mr.SEMIRINGS:
            Y = M.spmm(X, s, transpose=col)
            want = torch.empty((kc, ny), dtype=tdt, device="cuda")
            for c in range(kc):
                M.mxv(X[:, c].contiguous(), s, transpose=col, out=want[c])
            torch.cuda.synchronize()
            equal[f"{s}_{'cols' if col else 'rows'}"] = _same(Y.t().contiguous(), want, s)
    r["equal"] = equal
    r["all_equal"] = all(equal.values())
    rp, ci, v = M.export_csr()
    # the heaviest line: the tile row with the most entries, alone (two positional selects), timed at k = 1 and 4 against mxv
    tr_nnz = np.add.reduceat(np.diff(rp), np.arange(0, M.rows, 16)) if M.rows else np.zeros(1, np.int64)
    t0 = int(np.argmax(tr_nnz))
    H = M.select("row_gt", 16 * t0 - 1).select("row_le", 16 * t0 + 15)
    heavy = dict(tile_row=t0, entries=int(tr_nnz[t0]), longest_row=int(np.diff(rp)[16 * t0:16 * t0 + 16].max()))
    for k in (1, 4):
        X = torch.from_numpy(rng.standard_normal((M.cols, k)).astype(M.dtype)).cuda()
        Xs = torch.from_numpy(rng.standard_normal((M.cols, k + 1)).astype(M.dtype)).cuda()[:, :k]   # a column slice: the spmm kernel
        Y = torch.empty((M.rows, k), dtype=tdt, device="cuda")
        xc = [X[:, c].contiguous() for c in range(k)]
        yc = torch.empty((k, M.rows), dtype=tdt, device="cuda")
        heavy[f"k{k}_spmm_kernel_ms"] = round(_kernel_ms(ctx, lambda: H.spmm(Xs, out=Y), passes, warmup), 4)
        heavy[f"k{k}_mxv_kernel_ms"] = round(_kernel_ms(ctx, lambda: [H.mxv(xc[c], out=yc[c]) for c in range(k)], passes, warmup), 4)
    H.close()
    r["heaviest_line"] = heavy
    r["timing"] = {}
    for k in ks:
        t = {}
        for col, s in ((False, "plus_times"), (True, "plus_times"), (False, "min_plus")):
            nx, ny = (M.rows, M.cols) if col else (M.cols, M.rows)
            X = torch.from_numpy(rng.standard_normal((nx, k)).astype(M.dtype)).cuda()
            Y = torch.empty((ny, k), dtype=tdt, device="cuda")
            xc = [X[:, c].contiguous() for c in range(k)]
            yc = torch.empty((k, ny), dtype=tdt, device="cuda")
            f = (lambda X=X, Y=Y, s=s, col=col: M.spmm(X, s, transpose=col, out=Y))
            km = _kernel_ms(ctx, f, passes, warmup)
            nb = _bytes(M, col, vb, k)
            e = dict(kernel_ms=round(km, 4), wall_ms=round(_wall(f, ctx, passes, warmup), 4), bytes=nb, hbm_frac=_frac(nb, km),
                     gathered_bytes=int(M.nnz * k * vb))
            fm = (lambda s=s, col=col, xc=xc, yc=yc: [M.mxv(xc[c], s, transpose=col, out=yc[c]) for c in range(k)])
            e["k_mxv_kernel_ms"] = round(_kernel_ms(ctx, fm, passes, warmup), 4)
            e["speedup_vs_k_mxv"] = round(e["k_mxv_kernel_ms"] / km, 2) if km > 0 else 0.0
            t[f"{s}_{'cols' if col else 'rows'}"] = e
        # (b) rocSPARSE through torch: CSR @ dense block, rows orientation
        try:
            A = torch.sparse_csr_tensor(torch.from_numpy(rp.astype(np.int64)), torch.from_numpy(ci.astype(np.int64)),
                                        torch.from_numpy(v), size=(M.rows, M.cols)).cuda()
            X = torch.from_numpy(rng.standard_normal((M.cols, k)).astype(M.dtype)).cuda()
            for _ in range(warmup):
                A @ X
            ev = []
            for _ in range(passes):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                A @ X
                e1.record()
                e1.synchronize()
                ev.append(e0.elapsed_time(e1))
            t["torch_csr_spmm_ms"] = round(statistics.median(ev), 4)
            del A
        except Exception as ex:   # (not every torch build runs CSR @ dense on the device)
            t["torch_csr_spmm_ms"] = f"{type(ex).__name__}: {ex}"
        # (c) the plan route: X as an n x k tiling storing every entry, the warm repeat pass alone
        if k <= 16:
            n = M.cols
            jj, cc = np.meshgrid(np.arange(n, dtype=np.int32), np.arange(k, dtype=np.int32), indexing="ij")
            XD = pkg.Tiled.from_coo(ctx, n, k, jj.ravel(), cc.ravel(), rng.standard_normal(n * k), dtype=M.dtype)
            p = pkg.CPlan(ctx, M, XD)
            p.spgemm()
            t["plan_route_warm_pass_ms"] = round(_wall(lambda: p.spgemm(), ctx, passes, warmup), 4)
            p.close()
            XD.close()
        r["timing"][str(k)] = t
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="")
    ap.add_argument("--ks", default="1,4,16,64")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pkg = g.load_package()
    standins = importlib.import_module("pem_spgemm_amd.standins")
    import torch
    torch.cuda.is_available()
    names = a.only.split(",") if a.only else list(DEFAULT)
    ks = [int(x) for x in a.ks.split(",")]
    stream = torch.cuda.Stream()   # (torch's default stream is the null stream: the context and torch share this one instead)
    torch.cuda.set_stream(stream)
    ctx = pkg.Context(0, stream=stream.cuda_stream)
    results = {}
    for name in names:
        base = name[:-2] if name.endswith("^2") else name
        rows, cols, I, J, V = standins.make(base, 1.0)
        for dt in (np.float64, np.float32):
            A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=dt)
            M = A
            if name.endswith("^2"):
                plan = pkg.CPlan(ctx, A, A)
                plan.spgemm()
                M = pkg.Tiled.from_cplan(plan)
                plan.close()
            key = f"{name} {np.dtype(dt).name}"
            r = one_matrix(pkg, torch, ctx, M, ks, a.passes, a.warmup)
            results[key] = r
            print(f"{key:>24} nnz {r['nnz']:>10} tiles {r['ntiles']:>9} | all equal to mxv per column {r['all_equal']}", flush=True)
            h = r["heaviest_line"]
            print(f"{'':>24} heaviest tile row {h['tile_row']}: {h['entries']} entries, longest row {h['longest_row']} | k=1 spmm kernel "
                  f"{h['k1_spmm_kernel_ms']:.3f} ms, mxv {h['k1_mxv_kernel_ms']:.3f} ms | k=4 spmm {h['k4_spmm_kernel_ms']:.3f} ms, 4 mxv "
                  f"{h['k4_mxv_kernel_ms']:.3f} ms", flush=True)
            for k, t in r["timing"].items():
                line = f"{'':>24} k={k:>3}"
                for c in ("plus_times_rows", "plus_times_cols", "min_plus_rows"):
                    e = t[c]
                    line += (f" | {c} {e['kernel_ms']:.3f} ms (wall {e['wall_ms']:.3f}, {e['hbm_frac']:.2f} of 8 TB/s, gathered "
                             f"{e['gathered_bytes'] / 1e6:.0f} MB; k mxv {e['k_mxv_kernel_ms']:.3f} ms, x{e['speedup_vs_k_mxv']:.1f})")
                tc = t["torch_csr_spmm_ms"]
                line += f" | torch CSR @ X {tc:.3f} ms" if isinstance(tc, float) else f" | torch CSR @ X: {tc}"
                if "plan_route_warm_pass_ms" in t:
                    line += f" | plan route warm pass {t['plan_route_warm_pass_ms']:.3f} ms"
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
