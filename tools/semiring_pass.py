"""Step 3 under each semiring (pem_cplan_set_semiring) against plus-times on the same plan.

    python tools/semiring_pass.py [--rounds 20] [--warmup 3] [--only webbase-1M,...] [--out result.json]

Per workload, on the seeded stand-ins: one plan, one symbolic pass; then
  first, a check: C under every semiring other than plus-times equals tests/semiringref.py's numpy statement -- structure exact,
  values exact (min/max with -0 == +0) -- and plus-times after the round trip is bit-identical to the first pass's C.  cage15's C
  (~11 GB) is checked on its first 1/32 of tile rows (a plan of its own over that range);
  then --rounds rounds, each running pem_spgemm_step3 once under every semiring in turn (the order rotates per round), after
  --warmup such rounds; the library's step-3 event span of each call is collected and the medians are reported, with each
  semiring's ratio to plus-times.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402
import semiringref as sr  # noqa: E402

WORKLOADS = [("webbase-1M", False), ("webbase-1M-r2", False), ("scircuit", False), ("mc2depi", True), ("cage15", False)]


def _check(pkg, ctx, A, B, ops, lo, hi):
    """every semiring on tile rows [lo, hi): exact against the numpy statement"""
    arp, aci, av = ops[0]
    r0, r1 = 16 * lo, min(16 * hi, len(arp) - 1)
    sl = (arp[r0:r1 + 1] - arp[r0], aci[arp[r0]:arp[r1]], av[arp[r0]:arp[r1]])
    plan = pkg.CPlan(ctx, A, B, lo, hi)
    plan.spgemm()
    first = plan.export_csr()
    for s in sr.NEW:
        plan.set_semiring(s)
        plan.step3()
        rp, ci, v = plan.export_csr()
        wrp, wci, wv = sr.spgemm(sl, ops[1], ops[2], s)
        if not (np.array_equal(rp, wrp) and np.array_equal(ci, wci) and np.array_equal(ci, first[1]) and sr.same_values(v, wv)):
            raise SystemExit(f"semiring_pass: C under {s} differs from the numpy statement on tile rows [{lo}, {hi})")
        del rp, ci, v, wrp, wci, wv
    plan.set_semiring("plus_times")
    plan.step3()
    if not np.array_equal(plan.export_csr()[2].view(np.uint64), first[2].view(np.uint64)):
        raise SystemExit("semiring_pass: plus-times after the round trip differs from the first pass")
    plan.close()


def run(pkg, standins, name, aat, rounds, warmup):
    rows, cols, I, J, V = standins.make(name, 1.0)
    ctx = pkg.Context(0)
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    B = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, True) if aat else A
    a_csr = sr.coo_to_csr(rows, cols, I, J, V)
    ops = (a_csr, sr.transpose_csr(rows, cols, *a_csr) if aat else a_csr, rows if aat else cols)
    hi = A.tile_rows // 32 if name == "cage15" else A.tile_rows
    _check(pkg, ctx, A, B, ops, 0, hi)
    del ops, a_csr
    plan = pkg.CPlan(ctx, A, B)
    plan.spgemm()
    info = plan.info()
    times = {s: [] for s in sr.SEMIRINGS}
    for rnd in range(warmup + rounds):
        order = sr.SEMIRINGS[rnd % len(sr.SEMIRINGS):] + sr.SEMIRINGS[:rnd % len(sr.SEMIRINGS)]
        for s in order:
            plan.set_semiring(s)
            plan.step3()
            if rnd >= warmup:
                times[s].append(ctx.timings()["step3_ms"])
    med = {s: statistics.median(t) for s, t in times.items()}
    out = dict(workload=name, product="A*A^T" if aat else "A^2", nnz=int(A.nnz), nnz_c=info["nnz_c"], ntiles_c=info["ntiles_c"],
               npairs=info["npairs"], checked_rows=f"tile rows [0, {hi}) of {A.tile_rows}", exact=True,
               step3_median_ms=med, step3_min_ms={s: min(t) for s, t in times.items()},
               ratio_to_plus_times={s: med[s] / med["plus_times"] for s in sr.SEMIRINGS}, rounds=rounds)
    plan.close()
    if aat:
        B.close()
    A.close()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated workload names (default: all five)")
    ap.add_argument("--out", default="", help="also write the results as JSON here")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("semiring_pass: no GPU (this tool measures on the device only)")
    pkg = g.load_package()
    standins = importlib.import_module("pem_spgemm_amd.standins")
    only = set(filter(None, a.only.split(",")))
    res = []
    print(f"{'workload':>14} {'product':>6} {'nnz_c':>11}  step 3 median ms (ratio to plus_times): " + "  ".join(f"{s}" for s in sr.SEMIRINGS))
    for name, aat in WORKLOADS:
        if only and name not in only:
            continue
        r = run(pkg, standins, name, aat, a.rounds, a.warmup)
        res.append(r)
        cells = "  ".join(f"{r['step3_median_ms'][s]:.3f} ({r['ratio_to_plus_times'][s]:.2f})" for s in sr.SEMIRINGS)
        print(f"{r['workload']:>14} {r['product']:>6} {r['nnz_c']:>11}  {cells}", flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(rounds=a.rounds, warmup=a.warmup, results=res), f, indent=1)


if __name__ == "__main__":
    main()
