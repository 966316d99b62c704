"""Extract and transpose on the device (pem_tiled_extract, pem_tiled_transpose, their refreshes) against the two routes a user had.

    python tools/extract_pass.py [--passes 10] [--warmup 2] [--only webbase-1M,...] [--out profiles/extract_pass.json]

Per workload (seeded stand-ins; C = A^2 as a tiling by pem_tiled_from_cplan; host clock around call plus synchronise; medians over
--passes after --warmup, with the spread of the repeats as (min, max)):
  perm        a random symmetric permutation C(p, p)
  middle      the contiguous middle half of rows and columns
  rows10      a random 10 % row sample, all columns
  both10      that sample on both sides
  transpose   C^T
and the refresh of each (pem_tiled_set_values_from_extract / _from_transpose) after new values of C.  Every result is first compared,
array for array, with pem_tiled_from_coo of tests/extractref.py's result on the exported C; every refresh with a fresh build.
Baselines, timed in the same process and alternating with the device call:
  (a) the host route: pem_tiled_export_csr, scipy indexing, pem_tiled_from_csr (every fifth pass: it is seconds long);
  (b) the device route before this operation: P*C*Q as two plans plus pem_tiled_from_cplan, the selection tilings P and Q built outside
      the timed window (for transpose: pem_tiled_from_coo(.., transpose = 1) of the exported entries, the only route there was).
The split of one device call between the new kernels (ex_*, chain_*_t), the scans and sort, and derive_tiled comes from the library's
per-kernel events (pem_set_kernel_profiling).
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
import extractref as ex  # noqa: E402

DEFAULT = ("webbase-1M", "webbase-1M-r2", "scircuit")
ARRAYS = ("tile_keys", "tile_nnz_ptr", "masks", "rowptr", "rowcolidx", "vals", "masks_t", "tile_rowptr", "tile_colidx", "tile_colptr",
          "tile_rowidx", "tile_offsets")
INFO = ("rows", "cols", "nnz", "tile_rows", "tile_cols", "ntiles", "value_bytes")


def _ms(fn, ctx):
    ctx.synchronize()
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    t = (time.perf_counter() - t0) * 1e3
    if hasattr(out, "close"):
        out.close()
    return t


def _stat(ts):
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4), n=len(ts))


def _alternating(ctx, fns, passes, warmup, every):
    """fns: name -> callable, timed in turn inside one loop; every[name] = k times the name only on every k-th pass"""
    ts = {k: [] for k in fns}
    for i in range(warmup + passes):
        for k, fn in fns.items():
            if i >= warmup and (i - warmup) % every.get(k, 1):
                continue
            if i < warmup and every.get(k, 1) > 1 and i > 0:
                continue
            t = _ms(fn, ctx)
            if i >= warmup:
                ts[k].append(t)
    return {k: _stat(v) for k, v in ts.items() if v}


def _kernel_split(ctx, fn):
    ctx.reset_kernel_stats()
    ctx.set_kernel_profiling(True)
    out = fn()
    ctx.synchronize()
    ctx.set_kernel_profiling(False)
    st = ctx.kernel_stats()
    if hasattr(out, "close"):
        out.close()
    split = dict(new_kernels_ms=0.0, scans_and_sort_ms=0.0, derive_and_rest_ms=0.0)
    for k, v in st.items():
        if k.startswith("ex_") or k in ("chain_count_t_kernel", "chain_gather_t_kernel", "chain_cmap_kernel"):
            split["new_kernels_ms"] += v["total_ms"]
        elif k.startswith("scan") or k.startswith("rs_"):
            split["scans_and_sort_ms"] += v["total_ms"]
        else:
            split["derive_and_rest_ms"] += v["total_ms"]
    return {k: round(v, 4) for k, v in split.items()}, {k: round(v["total_ms"], 4) for k, v in st.items()}


def _same_tiling(x, y):
    if any(getattr(x, k) != getattr(y, k) for k in INFO):
        return False
    for k in ARRAYS:
        a, b = x.array(k), y.array(k)
        if a.dtype.kind == "f":
            a, b = a.view(np.uint64), b.view(np.uint64)
        if not np.array_equal(a, b):
            return False
    return True


def one_case(pkg, ctx, C, coo, key, RI, CJ, passes, warmup):
    import scipy.sparse as sp
    n = C.rows
    transpose = key == "transpose"
    make = (lambda: C.transpose()) if transpose else (lambda: C.extract(RI, CJ))
    R = make()
    if transpose:
        want = pkg.Tiled.from_coo(ctx, n, n, *coo, transpose=True)
    else:
        ni, nj, oi, oj, ov = ex.extract(n, n, *coo, RI, CJ)
        want = pkg.Tiled.from_coo(ctx, ni, nj, oi, oj, ov)
    equal = _same_tiling(R, want)
    want.close()

    def host():
        rp, ci, v = C.export_csr()
        S = sp.csr_matrix((v, ci, rp), shape=(n, n))
        if transpose:
            S = S.T.tocsr()
        else:
            if RI is not None:
                S = S[RI]
            if CJ is not None:
                S = S[:, CJ]
            S = sp.csr_matrix(S)
        S.sort_indices()
        return pkg.Tiled.from_csr(ctx, S.shape[0], S.shape[1], S.indptr, S.indices, S.data)

    if transpose:
        def device_before():
            rp, ci, v = C.export_csr()
            return pkg.Tiled.from_coo(ctx, n, n, np.repeat(np.arange(n, dtype=np.int32), np.diff(rp)), ci, v, transpose=True)
    else:
        P = None if RI is None else pkg.Tiled.from_coo(ctx, *ex.selection(len(RI), n, RI, left=True))
        Q = None if CJ is None else pkg.Tiled.from_coo(ctx, *ex.selection(len(CJ), n, CJ, left=False))

        def device_before():
            X, made = C, []
            for L, Rr in ((P, None), (None, Q)):
                if L is None and Rr is None:
                    continue
                plan = pkg.CPlan(ctx, L if L is not None else X, X if L is not None else Rr)
                plan.spgemm()
                X = pkg.Tiled.from_cplan(plan)
                plan.close()
                made.append(X)
            for t in made[:-1]:
                t.close()
            return X

    t = _alternating(ctx, dict(device=make, device_before=device_before, host=host), passes, warmup, dict(host=5))
    split, kern = _kernel_split(ctx, make)
    # the refresh, after new values of C, against a fresh build
    C.set_values(np.random.default_rng(len(key)).normal(size=C.nnz))
    refresh = (lambda: R.set_values_from_transpose(C)) if transpose else (lambda: R.set_values_from_extract(C))
    refresh()   # (first call: builds the map)
    ctx.synchronize()
    F = make()
    refresh_equal = _same_tiling(R, F)
    F.close()
    tr = _alternating(ctx, dict(refresh=refresh, fresh=make), passes, warmup, {})
    out = dict(nnz=R.nnz, ntiles=R.ntiles, shape=[R.rows, R.cols], equal=equal, refresh_equal=refresh_equal, **t, kernel_split=split,
               kernels=kern, refresh=tr["refresh"], fresh_build=tr["fresh"])
    d, b = t["device"], t["device_before"]
    out["faster_than_device_route_beyond_spread"] = bool(d["max_ms"] < b["min_ms"])
    R.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="")
    ap.add_argument("--cases", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pkg = g.load_package()
    standins = importlib.import_module("pem_spgemm_amd.standins")
    import torch
    torch.cuda.is_available()
    names = a.only.split(",") if a.only else list(DEFAULT)
    results = {}
    for name in names:
        rows, cols, I, J, V = standins.make(name, 1.0)
        ctx = pkg.Context(0)
        A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
        plan = pkg.CPlan(ctx, A, A)
        plan.spgemm()
        C = pkg.Tiled.from_cplan(plan)
        plan.close()
        rng = np.random.default_rng(7)
        n = C.rows
        p = rng.permutation(n).astype(np.int32)
        mid = np.arange(n // 4, n // 4 + n // 2, dtype=np.int32)
        smp = rng.choice(n, n // 10, replace=False).astype(np.int32)
        cases = dict(perm=(p, p), middle=(mid, mid), rows10=(smp, None), both10=(smp, smp), transpose=(None, None))
        r = dict(rows=rows, nnz_a=A.nnz, nnz_c=C.nnz, ntiles_c=C.ntiles)
        for key, (RI, CJ) in cases.items():
            if a.cases and key not in a.cases.split(","):
                continue
            rp, ci, v = C.export_csr()
            coo = (np.repeat(np.arange(n, dtype=np.int32), np.diff(rp)), ci, v)
            x = r[key] = one_case(pkg, ctx, C, coo, key, RI, CJ, a.passes, a.warmup)
            print(f"{name:>14} {key:>9}: nnz {x['nnz']:>10} tiles {x['ntiles']:>9} equal {x['equal']} | device {x['device']['median_ms']:.3f} ms "
                  f"({x['device']['min_ms']:.3f} .. {x['device']['max_ms']:.3f}; new kernels {x['kernel_split']['new_kernels_ms']:.3f}, scans + sort "
                  f"{x['kernel_split']['scans_and_sort_ms']:.3f}, derive_tiled + rest {x['kernel_split']['derive_and_rest_ms']:.3f}) | device route "
                  f"before {x['device_before']['median_ms']:.3f} ms ({x['device_before']['min_ms']:.3f} .. {x['device_before']['max_ms']:.3f}) | "
                  f"host route {x['host']['median_ms']:.1f} ms | refresh {x['refresh']['median_ms']:.3f} ms (equal {x['refresh_equal']}) vs fresh "
                  f"{x['fresh_build']['median_ms']:.3f} ms | faster than the device route beyond the spread: "
                  f"{x['faster_than_device_route_beyond_spread']}", flush=True)
        results[name] = r
        C.close()
        A.close()
        ctx.close()
        if a.out:   # (after every workload: a run that is cut short keeps what it measured)
            with open(a.out, "w") as f:
                json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
