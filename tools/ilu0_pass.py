"""ILU(0) on the device (pem_tiled_ilu0) on the three orderings tools/trsv_pass.py builds, against the solves that share its
dependencies.

    python tools/ilu0_pass.py [--passes 7] [--warmup 2] [--scale 1.0] [--out profiles/ilu0_pass.json]

The matrix: trsv_pass's -- the seeded webbase-1M stand-in's off-diagonal pattern, symmetrised, standard normal values, a dominant
diagonal -- in fp64, three times with the same n:
  natural      the stand-in's own numbering
  coloured     the same matrix after a greedy colouring, reordered on the device by extract(p, p)
  tridiagonal  the worst case of the same n: every tile row waits for the one before
Per matrix, trsv_pass's method (warm, the median of --passes host clocks around a call that ends in a synchronise):
  build        A.ilu0(): structure clone, schedule, vals_t map and the factorisation (it waits by itself)
  refresh      F.set_values_from_ilu0(A): the factorisation alone, levels and launches from F.ilu0_info(), also per level
  lu_solve     the lower (unit) + upper trsv pair on F: the same dependencies with far less work -- the yardstick
  mxv          one mxv on F: the same bytes with no dependencies
The refresh must reproduce the build bit for bit, and the number of zero pivots is recorded.  A vendor csrilu0 column is absent: this
tool binds no vendor library.
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
from trsv_pass import _median, _wall, greedy_colouring, symmetric_problem, with_diagonal  # noqa: E402


def _stats(t):
    med, lo, hi = t
    return dict(median=round(med, 4), min=round(lo, 4), max=round(hi, 4))


def measure(torch, ctx, A, label, passes, warmup):
    n = A.rows
    r = dict(n=n, nnz=A.nnz, ntiles=A.ntiles, dtype=A.dtype.name)
    ctx.trsv_split(False)
    keep = []

    def build():
        for F in keep:
            F.close()
        keep[:] = [A.ilu0()]

    r["build_ms"] = _stats(_median(build, ctx, passes, warmup))
    F = keep[0]
    first = F.array("vals")
    info = F.ilu0_info()
    r.update(levels=info["levels"], launches=info["launches"], max_width=info["max_width"], merge_width=info["merge_width"],
             zero_pivots=info["zero_pivots"])
    med, lo, hi = _median(lambda: F.set_values_from_ilu0(A), ctx, passes, warmup)
    r["refresh_ms"] = _stats((med, lo, hi))
    r["refresh_us_per_level"] = round(1e3 * med / max(1, info["levels"]), 3)
    r["refresh_equals_build"] = bool(np.array_equal(F.array("vals").view(np.uint64), first.view(np.uint64)))
    b = torch.from_numpy(np.random.default_rng(11).standard_normal(n)).cuda()
    z, work = torch.empty_like(b), torch.empty_like(b)
    F.lu_solve(b, out=z, work=work)   # (both schedules)
    r["lu_solve_ms"] = _stats(_median(lambda: F.lu_solve(b, out=z, work=work), ctx, passes, warmup))
    y = torch.empty_like(b)
    F.mxv(b, out=y)
    r["mxv_ms"] = _stats(_median(lambda: F.mxv(b, out=y), ctx, passes, warmup))
    r["rocsparse_csrilu0"] = "absent (this tool binds no vendor library)"
    F.close()
    print(f"{label:>11} n {n} nnz {r['nnz']} | levels {r['levels']} launches {r['launches']} max width {r['max_width']} | build "
          f"{r['build_ms']['median']:.3f} ms | refresh {r['refresh_ms']['median']:.3f} ms ({r['refresh_us_per_level']:.2f} us per level), same "
          f"bits {r['refresh_equals_build']} | lower + upper trsv {r['lu_solve_ms']['median']:.3f} ms | mxv {r['mxv_ms']['median']:.3f} ms | zero "
          f"pivots {r['zero_pivots']}", flush=True)
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
        raise SystemExit("ilu0_pass: no GPU (this tool measures on the device only)")
    stream = torch.cuda.Stream()   # (torch's default stream is the null stream: the context and torch share this one instead)
    torch.cuda.set_stream(stream)
    ctx = pkg.Context(0, stream=stream.cuda_stream)
    n, I, J, V = symmetric_problem(standins, a.scale)
    results = dict(workload=f"webbase-1M stand-in (scale {a.scale}), symmetrised pattern, dominant diagonal, fp64", passes=a.passes,
                   warmup=a.warmup)

    def save():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(results, f, indent=1)

    S = pkg.Tiled.from_coo(ctx, n, n, I, J, V)
    results["natural"] = measure(torch, ctx, S, "natural", a.passes, a.warmup)
    save()
    t0 = time.perf_counter()
    colour = greedy_colouring(n, I.astype(np.int64), J.astype(np.int64))
    p = np.argsort(colour, kind="stable").astype(np.int32)
    results["colouring"] = dict(colours=int(colour.max()) + 1, host_seconds=round(time.perf_counter() - t0, 2))
    R = S.extract(p, p)
    S.close()
    results["coloured"] = measure(torch, ctx, R, "coloured", a.passes, a.warmup)
    save()
    R.close()
    i = np.arange(1, n, dtype=np.int64)
    _, bi, bj, bv = with_diagonal(n, np.concatenate([i, i - 1]), np.concatenate([i - 1, i]), np.random.default_rng(8))
    B = pkg.Tiled.from_coo(ctx, n, n, bi, bj, bv)
    results["tridiagonal"] = measure(torch, ctx, B, "tridiagonal", a.passes, a.warmup)
    B.close()
    ctx.close()
    save()


if __name__ == "__main__":
    main()
