"""Chained products: a plan's C turned into the next operand on the device (pem_tiled_from_cplan) against today's host route.

    python tools/chain_pass.py [--passes 10] [--warmup 2] [--only webbase-1M,...] [--out result.json]

Per workload, on the seeded stand-ins (host clock around work that ends in a device synchronisation, medians over --passes):
  (1) conversion of C: pem_tiled_from_cplan untransposed and transposed, against pem_c_export_csr + pem_tiled_from_csr (the export
      route).  Before any timing the three tilings are compared with the export route's, array for array (C^T against
      pem_tiled_from_coo(transpose = 1) of the exported COO).  The kernels' device time comes from the library's per-kernel events,
      and the achieved bandwidth counts the compulsory 25 B per fp64 entry (c_vals read; vals, vals_t, rowcolidx written).
  (2) the chained product A^2 * A, with C of A^2 as the left operand; PEM_E_OVERFLOW (C beyond int32) or PEM_E_NOMEM is reported
      as not run.
  (3) Galerkin P^T (A P) on mc2depi, P aggregating 16 consecutive rows: after new values of A, the refreshed chain
      (set_values_device(A), step 3 of A P, set_values_from_cplan, step 3 of P^T (A P)) against a rebuild through export and
      re-conversion (step 3 of A P, export, from_csr, a new plan of P^T (A P), pem_spgemm).  Both results are compared first.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

WORKLOADS = [("webbase-1M", False), ("webbase-1M-r2", False), ("scircuit", False), ("mc2depi", True), ("cage15", False)]
DEFAULT = ("webbase-1M", "webbase-1M-r2", "scircuit", "mc2depi")   # cage15 (C of ~10^9 entries) only with --only: its host-side equality check needs tens of GB
COMPULSORY_B = 25   # fp64: 8 B of c_vals read, 8 + 8 + 1 B of vals, vals_t and rowcolidx written
ARRAYS = ("tile_keys", "tile_nnz_ptr", "masks", "rowptr", "rowcolidx", "vals", "masks_t", "tile_rowptr", "tile_colidx", "tile_colptr",
          "tile_rowidx", "tile_offsets")
PEM_E_OVERFLOW, PEM_E_NOMEM = -4, -3


def _ms(fn, ctx):
    ctx.synchronize()
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _med(xs):
    return statistics.median(xs) if xs else None


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        a, b = a.view(np.uint64), b.view(np.uint64)
    return a.shape == b.shape and np.array_equal(a, b)


def _reconvert(pkg, ctx, plan, transpose):
    rows, cols = plan.A.rows, plan.B.cols
    if transpose:
        r, c, v = plan.export_coo()
        return pkg.Tiled.from_coo(ctx, rows, cols, r, c, v, True)
    rp, ci, v = plan.export_csr()
    return pkg.Tiled.from_csr(ctx, rows, cols, rp, ci, v)


def _check(pkg, ctx, plan, label):
    for tr in (0, 1):
        got, want = pkg.Tiled.from_cplan(plan, tr), _reconvert(pkg, ctx, plan, tr)
        for k in ("rows", "cols", "nnz", "ntiles"):
            assert getattr(got, k) == getattr(want, k), (label, tr, k)
        for a in ARRAYS:
            assert _same(got.array(a), want.array(a)), (label, tr, a)
        got.close()
        want.close()


def _kernel_ms(ctx, fn):
    """device time of every kernel fn launches (the library's per-kernel events)"""
    ctx.reset_kernel_stats()
    ctx.set_kernel_profiling(True)
    fn()
    ctx.synchronize()
    ctx.set_kernel_profiling(False)
    st = ctx.kernel_stats()
    return sum(v["total_ms"] for v in st.values()), {k: round(v["total_ms"], 4) for k, v in st.items()}


def conversion(pkg, ctx, name, plan, passes, warmup):
    nnz = plan.info()["nnz_c"]
    _check(pkg, ctx, plan, name)
    res = dict(nnz_c=nnz)
    for tr in (0, 1):
        for _ in range(warmup):
            pkg.Tiled.from_cplan(plan, tr).close()
        xs = []
        for _ in range(passes):
            ms, T = _ms(lambda: pkg.Tiled.from_cplan(plan, tr), ctx)
            xs.append(ms)
            T.close()
        kms, per = _kernel_ms(ctx, lambda: pkg.Tiled.from_cplan(plan, tr).close())
        res[f"from_cplan_t{tr}"] = dict(median_ms=_med(xs), kernels_ms=kms, kernels=per,
                                        tb_s_wall=COMPULSORY_B * nnz / (_med(xs) * 1e-3) / 1e12,
                                        tb_s_kernels=COMPULSORY_B * nnz / (kms * 1e-3) / 1e12 if kms else None)
    xs = []
    for k in range(max(2, passes // 2) + 1):
        ms, T = _ms(lambda: _reconvert(pkg, ctx, plan, 0), ctx)
        if k:
            xs.append(ms)
        T.close()
    res["export_route"] = dict(median_ms=_med(xs))
    return res


def cube(pkg, ctx, A, plan, passes):
    T = pkg.Tiled.from_cplan(plan)
    try:
        p = pkg.CPlan(ctx, T, A)
        p.spgemm()
    except pkg.PemError as e:
        if e.status in (PEM_E_OVERFLOW, PEM_E_NOMEM):
            return dict(run=False, reason=str(e))
        raise
    xs = []
    for _ in range(passes):
        p.spgemm()
        xs.append(ctx.timings()["spgemm_wall_ms"])
    out = dict(run=True, nnz_c=p.info()["nnz_c"], pass_median_ms=_med(xs))
    p.close()
    T.close()
    return out


def galerkin(pkg, standins, torch, passes, warmup):
    rows, cols, I, J, V = standins.make("mc2depi", 1.0)
    order = np.argsort(I.astype(np.int64) * cols + J, kind="stable")
    n, nc = rows, (rows + 15) // 16
    PI = np.arange(n, dtype=np.int32)
    PJ = (PI // 16).astype(np.int32)
    ctx = pkg.Context(0)
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    P = pkg.Tiled.from_coo(ctx, n, nc, PI, PJ, np.ones(n))
    Pt = pkg.Tiled.from_coo(ctx, n, nc, PI, PJ, np.ones(n), True)
    ap = pkg.CPlan(ctx, A, P)
    ap.spgemm()
    AP = pkg.Tiled.from_cplan(ap)
    gp = pkg.CPlan(ctx, Pt, AP)
    gp.spgemm()
    rng = np.random.default_rng(77)
    vals = [torch.from_numpy(rng.uniform(-1, 1, len(I))[order]).to("cuda") for _ in range(2)]
    torch.cuda.synchronize()

    def chained(dV):
        A.set_values_device(dV, "row")
        ap.step3()
        AP.set_values_from_cplan(ap)
        gp.step3()

    def rebuild(dV):
        A.set_values_device(dV, "row")
        ap.step3()
        rp, ci, v = ap.export_csr()
        T = pkg.Tiled.from_csr(ctx, n, nc, rp, ci, v)
        p = pkg.CPlan(ctx, Pt, T)
        p.spgemm()
        return p, T

    chained(vals[1])
    p, T = rebuild(vals[1])
    for x, y in zip(gp.export_csr(), p.export_csr()):
        assert _same(x, y), "galerkin: refreshed chain differs from the rebuild"
    p.close()
    T.close()
    a, b = [], []
    for k in range(warmup + passes):
        ms, _ = _ms(lambda: chained(vals[k % 2]), ctx)
        if k >= warmup:
            a.append(ms)
        ms, pt = _ms(lambda: rebuild(vals[k % 2]), ctx)
        pt[0].close()
        pt[1].close()
        if k >= warmup:
            b.append(ms)
    info = dict(ap_nnz=ap.info()["nnz_c"], galerkin_nnz=gp.info()["nnz_c"], refreshed_chain_ms=_med(a), rebuild_ms=_med(b))
    ctx.close()
    return info


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
    only = set(a.only.split(",")) if a.only else set(DEFAULT)
    results = dict(workloads={}, galerkin=None)
    for name, aat in WORKLOADS:
        if name not in only:
            continue
        rows, cols, I, J, V = standins.make(name, 1.0)
        ctx = pkg.Context(0)
        A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
        B = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, True) if aat else A
        plan = pkg.CPlan(ctx, A, B)
        plan.spgemm()
        r = conversion(pkg, ctx, name, plan, a.passes, a.warmup)
        r["product"] = "A*A^T" if aat else "A^2"
        if not aat:
            r["cube"] = cube(pkg, ctx, A, plan, a.passes)
        results["workloads"][name] = r
        t0, t1, ex = r["from_cplan_t0"], r["from_cplan_t1"], r["export_route"]
        print(f"{name:>14} {r['product']:>5} C nnz {r['nnz_c']:>10}  from_cplan {t0['median_ms']:8.3f} ms (kernels {t0['kernels_ms']:7.3f} ms, "
              f"{t0['tb_s_kernels'] or 0:.2f} TB/s at 25 B)  transposed {t1['median_ms']:8.3f} ms (kernels {t1['kernels_ms']:7.3f})  "
              f"export + from_csr {ex['median_ms']:9.3f} ms", flush=True)
        if "cube" in r:
            c = r["cube"]
            print(f"{'':>14} A^2*A: " + (f"C nnz {c['nnz_c']}, pass {c['pass_median_ms']:.3f} ms" if c["run"] else f"not run ({c['reason']})"),
                  flush=True)
        plan.close()
        ctx.close()
    if "mc2depi" in only:
        results["galerkin"] = galerkin(pkg, standins, torch, a.passes, a.warmup)
        gl = results["galerkin"]
        print(f"galerkin mc2depi P^T(A P): refreshed chain {gl['refreshed_chain_ms']:.3f} ms, rebuild through export {gl['rebuild_ms']:.3f} ms", flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
