"""Masked products C<M> = A*B (pem_cplan_create_masked) against the unmasked pass on the same operands.

    python tools/masked_pass.py [--passes 20] [--warmup 3] [--only webbase-1M,...] [--out result.json]

Per workload, on the seeded stand-ins (M = A for the A^2 workloads -- triangle counting's mask; M = the pattern of the unmasked C
for mc2depi's A*A^T, so its complement is empty):
  first, a check: the masked C and the complement's C equal the unmasked C filtered by M (and by its complement) bit for bit,
  compared on the device (cage15 in eight tile-row slices: its unmasked C is ~11 GB);
  then medians over --passes warm passes (graph replay off; host clock around pem_spgemm, which ends in a device sync) of the
  unmasked pass, the masked pass and the complement pass, with the library's step 1/2/3 times of each;
  and the filter kernels' device times (per-kernel events, a loop of its own) with the bandwidth they reach counting 12 B per
  pair read (pair_col, pairs_a, pairs_b) and 12 B per kept pair written.
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

WORKLOADS = [("webbase-1M", False), ("webbase-1M-r2", False), ("scircuit", False), ("mc2depi", True), ("cage15", False)]
FILTER_KERNELS = ("mask_heads_kernel", "mask_count_kernel", "mask_compact_kernel")


def _stats(xs):
    return dict(median_ms=statistics.median(xs), mean_ms=statistics.fmean(xs), min_ms=min(xs), n=len(xs))


def _csr_dev(torch, ctx, p):
    i = p.info()
    rp = torch.empty(i["row_end"] - i["row_begin"] + 1, dtype=torch.int32, device="cuda")
    ci = torch.empty(i["nnz_c"], dtype=torch.int32, device="cuda")
    cv = torch.empty(i["nnz_c"], dtype=torch.float64, device="cuda")
    p.export_csr_device(rp.data_ptr(), ci.data_ptr(), cv.data_ptr())
    ctx.synchronize()
    return i["row_begin"], rp, ci, cv.view(torch.int64)


def _check(torch, pkg, ctx, A, B, M, m_keys, slices):
    """masked / complement C == unmasked C filtered, bit for bit, slice by slice"""
    bounds = np.linspace(0, A.tile_rows, slices + 1).astype(int)
    ncols = B.cols
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        u = pkg.CPlan(ctx, A, B, int(lo), int(hi))
        u.spgemm()
        r0, rp, ci, cv = _csr_dev(torch, ctx, u)
        u.close()
        rows = r0 + torch.repeat_interleave(torch.arange(len(rp) - 1, device="cuda", dtype=torch.int64), (rp[1:] - rp[:-1]).long())
        inm = torch.isin(rows * ncols + ci.long(), m_keys)
        for comp in (False, True):
            keep = ~inm if comp else inm
            p = pkg.CPlan(ctx, A, B, int(lo), int(hi), mask=M, complement=comp)
            p.spgemm()
            _, grp, gci, gcv = _csr_dev(torch, ctx, p)
            p.close()
            cnt = torch.bincount(rows[keep] - r0, minlength=len(rp) - 1)
            wrp = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(cnt, 0)])
            if not (torch.equal(grp.long(), wrp) and torch.equal(gci, ci[keep]) and torch.equal(gcv, cv[keep])):
                raise SystemExit(f"masked C (complement={comp}) differs from the filtered unmasked C in tile rows [{lo}, {hi})")
            del grp, gci, gcv, keep, cnt, wrp
        del rows, inm, rp, ci, cv
        torch.cuda.empty_cache()


def _passes(ctx, plan, passes, warmup):
    for _ in range(warmup):
        plan.spgemm()
    wall, s1, s2, s3 = [], [], [], []
    for _ in range(passes):
        plan.spgemm()
        t = ctx.timings()
        wall.append(t["spgemm_wall_ms"])
        s1.append(t["step1_ms"])
        s2.append(t["step2_ms"])
        s3.append(t["step3_ms"])
    return dict(pass_=_stats(wall), step1_ms=statistics.median(s1), step2_ms=statistics.median(s2), step3_ms=statistics.median(s3))


def run(pkg, standins, torch, name, aat, passes, warmup):
    rows, cols, I, J, V = standins.make(name, 1.0)
    ctx = pkg.Context(0)
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    B = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, True) if aat else A
    if aat:   # M = the pattern of A*A^T itself
        u = pkg.CPlan(ctx, A, B)
        u.spgemm()
        rp, ci, _ = u.export_csr()
        u.close()
        MI, MJ = np.repeat(np.arange(rows, dtype=np.int32), np.diff(rp)), ci
        M = pkg.Tiled.from_coo(ctx, rows, B.cols, MI, MJ, np.ones(len(MI)))
        del rp, ci
    else:
        MI, MJ, M = I, J, A
    m_keys = torch.from_numpy(MI.astype(np.int64) * B.cols + MJ.astype(np.int64)).to("cuda")
    _check(torch, pkg, ctx, A, B, M, m_keys, 8 if name == "cage15" else 1)
    del m_keys
    torch.cuda.empty_cache()
    out = dict(workload=name, product="A*A^T" if aat else "A^2", mask="pattern(A*A^T)" if aat else "A", nnz=int(A.nnz), mask_nnz=int(M.nnz),
               c_checked_bit_exact=True)
    for label, kw in (("unmasked", {}), ("masked", dict(mask=M)), ("complement", dict(mask=M, complement=True))):
        plan = pkg.CPlan(ctx, A, B, **kw)
        res = _passes(ctx, plan, passes, warmup)
        res.update({k: plan.info()[k] for k in ("ntiles_c", "npairs", "nnz_c", "npairs_all")})
        if kw:
            ctx.set_kernel_profiling(True)
            ctx.reset_kernel_stats()
            for _ in range(passes):
                plan.spgemm()
            ctx.synchronize()
            ks = ctx.kernel_stats()
            ctx.set_kernel_profiling(False)
            per = {k: ks[k]["total_ms"] / ks[k]["calls"] for k in FILTER_KERNELS if k in ks}
            fms = sum(per.values())
            moved = 12.0 * (unmasked_pairs + res["npairs"])          # the unmasked list read, the kept pairs written
            res.update(filter_kernels_ms=per, filter_ms=fms, filter_bytes=moved, filter_GBps=moved / (fms * 1e-3) / 1e9 if fms > 0 else 0.0)
        else:
            unmasked_pairs = res["npairs"]
        out[label] = res
        plan.close()
    if M is not A:
        M.close()
    if aat:
        B.close()
    A.close()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated workload names (default: all five)")
    ap.add_argument("--out", default="", help="also write the results as JSON here")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("masked_pass: no GPU (this tool measures on the device only)")
    pkg = g.load_package()
    standins = importlib.import_module("pem_spgemm_amd.standins")
    only = set(filter(None, a.only.split(",")))
    res = []
    for name, aat in WORKLOADS:
        if only and name not in only:
            continue
        r = run(pkg, standins, torch, name, aat, a.passes, a.warmup)
        res.append(r)
        u, m, c = r["unmasked"], r["masked"], r["complement"]
        print(f"{r['workload']:>14} {r['product']:>5}<{r['mask']}>  nnz_c {u['nnz_c']:>11} -> {m['nnz_c']:>10} (complement {c['nnz_c']:>11})  "
              f"pass {u['pass_']['median_ms']:8.3f} / masked {m['pass_']['median_ms']:8.3f} / complement {c['pass_']['median_ms']:8.3f} ms  "
              f"steps 1/2/3 {u['step1_ms']:.3f}/{u['step2_ms']:.3f}/{u['step3_ms']:.3f} -> {m['step1_ms']:.3f}/{m['step2_ms']:.3f}/{m['step3_ms']:.3f} "
              f"(complement {c['step1_ms']:.3f}/{c['step2_ms']:.3f}/{c['step3_ms']:.3f}) ms  "
              f"filter {m['filter_ms'] * 1e3:.1f} us = {m['filter_GBps']:.0f} GB/s (complement {c['filter_ms'] * 1e3:.1f} us = "
              f"{c['filter_GBps']:.0f} GB/s)", flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(passes=a.passes, warmup=a.warmup, results=res), f, indent=1)


if __name__ == "__main__":
    main()
