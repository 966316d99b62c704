"""Assign on the device (pem_tiled_assign and its refresh) against the host route a user had.

    python tools/assign_pass.py [--passes 10] [--warmup 2] [--only webbase-1M,...] [--out profiles/assign_pass.json]

Per workload (seeded stand-ins; C the stand-in's tiling, A = C(s, s) for a random sample s of 1/8 of the rows, so A is about as dense
as C; host clock around call plus synchronise; medians over --passes after --warmup, with the spread of the repeats as (min, max)):
  aligned     the block I = J = a tile-aligned range of 1/8 of the rows
  permuted    I = J = a random sample of 1/8 of the rows, in random order
each without an accum (C(I, J) = A), with plus (C(I, J) += A), and the refresh (pem_tiled_set_values_from_assign) after new values of
C and of A.  Every result is first compared, array for array, with pem_tiled_from_coo of tests/assignref.py's result on the exported
operands; every refresh with a fresh assign.  Baseline, timed in the same process and alternating with the device call (every fifth
pass: it is seconds long): the host route -- pem_tiled_export_csr of C and of A, the edit on the host (assignref), pem_tiled_from_coo.
The split of one device call between the stages comes from the library's per-kernel events (pem_set_kernel_profiling).
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as g  # noqa: E402
import assignref as ar  # noqa: E402
from extract_pass import _alternating, _same_tiling  # noqa: E402

DEFAULT = ("webbase-1M",)


def _coo(T):
    rp, ci, v = T.export_csr()
    return np.repeat(np.arange(T.rows, dtype=np.int32), np.diff(rp)), ci, v


def _kernel_split(ctx, fn):
    ctx.reset_kernel_stats()
    ctx.set_kernel_profiling(True)
    out = fn()
    ctx.synchronize()
    ctx.set_kernel_profiling(False)
    st = ctx.kernel_stats()
    out.close()
    split = dict(lists_and_map_ms=0.0, scatter_ms=0.0, region_drop_ms=0.0, merge_ms=0.0, scans_and_sort_ms=0.0, derive_and_rest_ms=0.0)
    for k, v in st.items():
        key = ("lists_and_map_ms" if k.startswith("as_") else "scatter_ms" if k.startswith("ex_") or k.startswith("chain_") else
               "region_drop_ms" if k.startswith("sel_") else "merge_ms" if k.startswith("ew_") else
               "scans_and_sort_ms" if k.startswith("scan") or k.startswith("rs_") else "derive_and_rest_ms")
        split[key] += v["total_ms"]
    return {k: round(v, 4) for k, v in split.items()}


def one_case(pkg, ctx, C, A, L, accum, passes, warmup):
    n = C.rows
    make = lambda: C.assign(A, L, L, accum=accum)   # noqa: E731
    Z = make()
    want = pkg.Tiled.from_coo(ctx, n, n, *ar.assign(n, n, _coo(C), _coo(A), L, L, accum))
    equal = _same_tiling(Z, want)
    want.close()

    def host():
        return pkg.Tiled.from_coo(ctx, n, n, *ar.assign(n, n, _coo(C), _coo(A), L, L, accum))

    t = _alternating(ctx, dict(device=make, host=host), passes, warmup, dict(host=5))
    split = _kernel_split(ctx, make)
    rng = np.random.default_rng(3)
    C.set_values(rng.normal(size=C.nnz))
    A.set_values(rng.normal(size=A.nnz))
    refresh = lambda: Z.set_values_from_assign(C, A)   # noqa: E731
    refresh()   # (first call: builds the map)
    ctx.synchronize()
    F = make()
    refresh_equal = _same_tiling(Z, F)
    F.close()
    tr = _alternating(ctx, dict(refresh=refresh, fresh=make), passes, warmup, {})
    out = dict(nnz=Z.nnz, ntiles=Z.ntiles, equal=equal, refresh_equal=refresh_equal, **t, kernel_split=split, refresh=tr["refresh"],
               fresh_build=tr["fresh"], host_over_device=round(t["host"]["median_ms"] / t["device"]["median_ms"], 1),
               host_over_refresh=round(t["host"]["median_ms"] / tr["refresh"]["median_ms"], 1))
    Z.close()
    return out


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
    results = {}
    for name in (a.only.split(",") if a.only else list(DEFAULT)):
        rows, cols, I, J, V = standins.make(name, 1.0)
        ctx = pkg.Context(0)
        C = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
        rng = np.random.default_rng(7)
        n, k = C.rows, C.rows // 8
        A = C.extract(np.sort(rng.choice(n, k, replace=False)).astype(np.int32), None)
        A = A.extract(None, np.sort(rng.choice(n, k, replace=False)).astype(np.int32))
        a0 = 16 * ((n // 3) // 16)
        lists = dict(aligned=np.arange(a0, a0 + k, dtype=np.int32), permuted=rng.choice(n, k, replace=False).astype(np.int32))
        r = dict(rows=rows, nnz_c=C.nnz, ntiles_c=C.ntiles, block=k, nnz_a=A.nnz)
        for lname, L in lists.items():
            for accum in (None, "plus"):
                key = f"{lname}_{accum or 'none'}"
                x = r[key] = one_case(pkg, ctx, C, A, L, accum, a.passes, a.warmup)
                print(f"{name:>14} {key:>14}: nnz {x['nnz']:>9} equal {x['equal']} | device {x['device']['median_ms']:.3f} ms "
                      f"({x['device']['min_ms']:.3f} .. {x['device']['max_ms']:.3f}; {x['kernel_split']}) | host route "
                      f"{x['host']['median_ms']:.1f} ms ({x['host_over_device']}x) | refresh {x['refresh']['median_ms']:.3f} ms (equal "
                      f"{x['refresh_equal']}; host route {x['host_over_refresh']}x) vs fresh {x['fresh_build']['median_ms']:.3f} ms", flush=True)
        results[name] = r
        ctx.close()
        if a.out:   # (after every workload: a run that is cut short keeps what it measured)
            with open(a.out, "w") as f:
                json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
