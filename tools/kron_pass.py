"""The Kronecker product on the device (pem_tiled_kron, pem_tiled_set_values_from_kron) against the route it replaces.

    python tools/kron_pass.py [--passes 10] [--warmup 2] [--only power10,...] [--out result.json]

Per workload (seeded stand-ins; host clock around work that ends in a device synchronisation, medians over --passes; kernel device
times from the library's per-kernel events):
  kron       Tiled.kron(A, B) on the device;
  refresh    set_values_from_kron after new values in A and B (first compared with a fresh kron);
  torch      the route available without it: the operands' (row, column, value) triples on the device (made once, outside the
             clock), the nnz(A) * nnz(B) triples expanded by broadcasting in torch, then pem_tiled_from_coo_device -- on a context that
             shares torch's stream, so nothing waits in between.  Its tiling is what kron's is compared with, array for array, and
             vals_t through mxv(transpose=True).
Workloads:
  power10            a 3 x 3 seed with 5 entries raised to the 10th Kronecker power by repeated kron of results (59 049 x 59 049,
                     9 765 625 entries): the last step seed^9 (x) seed is the timed call, the whole chain of nine is timed as well
  scircuit_x_d4      the scircuit stand-in (x) a dense 4 x 4
  i8_x_webbase       I_8 (x) the webbase-1M stand-in
  webbase_x_d2       the webbase-1M stand-in (x) a dense 2 x 2
Bytes (fp64): the payload kernel's nominal traffic -- per entry 13 B written (value, (r << 4) | c byte, tile-head scan) and 8 B read
(B's value; A's is read once per row segment), per tile of R 60 B (key, 16 row masks, offsets, tile_keys and tile_nnz_ptr) -- as a
fraction of 8 TB/s over kr_fill_kernel's time; the refresh moves 44 B per entry (the int2 map, vmap_t, two gathered values, two
written).
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

DEFAULT = ("power10", "scircuit_x_d4", "i8_x_webbase", "webbase_x_d2")
ARRAYS = ("tile_keys", "tile_nnz_ptr", "masks", "rowptr", "rowcolidx", "vals", "masks_t", "tile_rowptr", "tile_colidx", "tile_colptr",
          "tile_rowidx", "tile_offsets")
INFO = ("rows", "cols", "nnz", "tile_rows", "tile_cols", "ntiles", "value_bytes")


def _ms(fn, ctx):
    ctx.synchronize()
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _timed(fn, ctx, passes, warmup):
    ts = []
    for i in range(warmup + passes):
        t, out = _ms(fn, ctx)
        if i >= warmup:
            ts.append(t)
        if hasattr(out, "close"):
            out.close()
    return round(statistics.median(ts), 4)


def _kernels(ctx, fn):
    """device ms of one call by kernel name"""
    ctx.reset_kernel_stats()
    ctx.set_kernel_profiling(True)
    out = fn()
    ctx.synchronize()
    ctx.set_kernel_profiling(False)
    st = ctx.kernel_stats()
    if hasattr(out, "close"):
        out.close()
    return {k: round(v["total_ms"], 4) for k, v in st.items()}


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


def _same_vals_t(torch, ctx, x, y):
    """vals_t through its reader: mxv with transpose"""
    probe = torch.from_numpy(np.random.default_rng(3).normal(size=x.rows)).cuda()
    torch.cuda.synchronize()
    a, b = x.mxv(probe, transpose=True), y.mxv(probe, transpose=True)
    ctx.synchronize()
    return torch.equal(a.view(torch.int64), b.view(torch.int64))


def _frac(nbytes, ms):
    return round(nbytes / (ms * 1e-3) / 8.0e12, 4) if ms > 0 else 0.0


def _triples(torch, T):
    """a tiling's entries as device tensors (int64 rows, int64 columns, values), in CSR order"""
    rp, ci, v = T.export_csr()
    I = np.repeat(np.arange(T.rows, dtype=np.int64), np.diff(rp))
    out = torch.from_numpy(I).cuda(), torch.from_numpy(ci.astype(np.int64)).cuda(), torch.from_numpy(v).cuda()
    torch.cuda.synchronize()
    return out


def _dense(pkg, ctx, n, rng):
    I, J = (x.ravel().astype(np.int32) for x in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    return pkg.Tiled.from_coo(ctx, n, n, I, J, rng.uniform(0.5, 1.5, n * n))


def _operands(pkg, ctx, name, standins):
    """(A, B, extra): the tilings of the timed kron, and for power10 the seed chain's description"""
    rng = np.random.default_rng(11)
    if name == "power10":
        seed = pkg.Tiled.from_coo(ctx, 3, 3, [0, 0, 1, 2, 2], [0, 1, 2, 0, 2], [0.9, 0.7, 0.6, 0.8, 0.5])
        K = seed
        for _ in range(8):
            K = pkg.Tiled.kron(K, seed)
        return K, seed
    if name == "scircuit_x_d4":
        return pkg.Tiled.from_coo(ctx, *standins.make("scircuit", 1.0)), _dense(pkg, ctx, 4, rng)
    if name == "i8_x_webbase":
        eye = pkg.Tiled.from_coo(ctx, 8, 8, np.arange(8), np.arange(8), np.ones(8))
        return eye, pkg.Tiled.from_coo(ctx, *standins.make("webbase-1M", 1.0))
    if name == "webbase_x_d2":
        return pkg.Tiled.from_coo(ctx, *standins.make("webbase-1M", 1.0)), _dense(pkg, ctx, 2, rng)
    raise SystemExit(f"unknown workload {name}")


def workload(pkg, torch, name, standins, passes, warmup):
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = pkg.Context(0, stream=stream.cuda_stream)
    A, B = _operands(pkg, ctx, name, standins)
    aI, aJ, aV = _triples(torch, A)
    bI, bJ, bV = _triples(torch, B)
    rows, cols, n = A.rows * B.rows, A.cols * B.cols, A.nnz * B.nnz

    def torch_route():
        P = (aI[:, None] * B.rows + bI[None, :]).reshape(-1).to(torch.int32)
        Q = (aJ[:, None] * B.cols + bJ[None, :]).reshape(-1).to(torch.int32)
        V = (aV[:, None] * bV[None, :]).reshape(-1)
        return pkg.Tiled.from_coo_device(ctx, rows, cols, n, P.data_ptr(), Q.data_ptr(), V.data_ptr(), False)

    dev = lambda: pkg.Tiled.kron(A, B)
    R, want = dev(), torch_route()
    res = dict(rows=rows, cols=cols, nnz_a=A.nnz, nnz_b=B.nnz, nnz=R.nnz, ntiles=R.ntiles)
    res["equal"] = _same_tiling(R, want) and _same_vals_t(torch, ctx, R, want)
    want.close()
    ks = _kernels(ctx, dev)
    nbytes = 21 * R.nnz + 60 * R.ntiles
    res["kernels_ms"] = ks
    res["kron"] = dict(device_ms=_timed(dev, ctx, passes, warmup), kron_kernels_ms=round(sum(v for k, v in ks.items() if k.startswith("kr_")), 4),
                       all_kernels_ms=round(sum(ks.values()), 4), fill_kernel_ms=round(sum(v for k, v in ks.items() if k.startswith("kr_fill")), 4),
                       bytes=int(nbytes))
    res["kron"]["hbm_frac_fill"] = _frac(nbytes, res["kron"]["fill_kernel_ms"])
    res["torch_route_ms"] = _timed(torch_route, ctx, max(2, passes // 2), 1)
    res["ratio"] = round(res["torch_route_ms"] / res["kron"]["device_ms"], 2)
    if name == "power10":
        def chain():
            K = B
            for _ in range(9):
                K2 = pkg.Tiled.kron(K, B)
                if K is not B:
                    K.close()
                K = K2
            return K
        res["chain_of_nine_ms"] = _timed(chain, ctx, max(2, passes // 2), 1)
    # ---- refresh ----
    rng = np.random.default_rng(1)
    R.set_values_from_kron(A, B)   # (first call: the map)
    A.set_values(rng.normal(size=A.nnz))
    B.set_values(rng.normal(size=B.nnz))
    R.set_values_from_kron(A, B)
    ctx.synchronize()
    F = dev()
    refresh = lambda: R.set_values_from_kron(A, B)
    rk = _kernels(ctx, refresh)
    r_ms = round(sum(rk.values()), 4)
    res["refresh"] = dict(equal=_same_tiling(R, F) and _same_vals_t(torch, ctx, R, F), device_ms=_timed(refresh, ctx, passes, warmup), kernel_ms=r_ms,
                          bytes=int(44 * R.nnz), hbm_frac_kernel=_frac(44 * R.nnz, r_ms))
    for x in (F, R, A, B):
        x.close()
    ctx.close()
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--passes", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--only", default="")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "kron_pass.json"))
    a = p.parse_args()
    pkg = g.load_package()
    standins = importlib.import_module("pem_spgemm_amd.standins")
    import torch
    torch.cuda.is_available()
    results = {}
    for name in a.only.split(",") if a.only else list(DEFAULT):
        r = results[name] = workload(pkg, torch, name, standins, a.passes, a.warmup)
        k, f = r["kron"], r["refresh"]
        print(f"{name}: {r['rows']} x {r['cols']}, nnz {r['nnz_a']} * {r['nnz_b']} = {r['nnz']}, tiles {r['ntiles']}", flush=True)
        print(f"  {'kron':>10}: equal {r['equal']}, {k['device_ms']:.3f} ms (kr_ kernels {k['kron_kernels_ms']:.3f} ms, all kernels {k['all_kernels_ms']:.3f} ms; "
              f"fill {k['fill_kernel_ms']:.3f} ms, {k['hbm_frac_fill']:.2f} of 8 TB/s) vs torch + from_coo_device {r['torch_route_ms']:.3f} ms: {r['ratio']}x", flush=True)
        if "chain_of_nine_ms" in r:
            print(f"  {'chain':>10}: seed -> seed^10 by nine krons {r['chain_of_nine_ms']:.3f} ms", flush=True)
        print(f"  {'refresh':>10}: equal {f['equal']}, {f['device_ms']:.4f} ms (kernel {f['kernel_ms']:.4f} ms, {f['hbm_frac_kernel']:.2f} of 8 TB/s)", flush=True)
        print("  kernels: " + ", ".join(f"{n} {ms:.3f}" for n, ms in sorted(r["kernels_ms"].items(), key=lambda x: -x[1])[:8]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
