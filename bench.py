#!/usr/bin/env python3
"""bench.py -- the reference's headline metric on MI355X: SpGEMM GFLOP/s = 2*flop / t, where t is
one pass of step1+step2+step3 (spgemm.cu:1136-1341, 1403) on a matrix already resident in
HBM in tiled form.

    python bench.py --gpus N --steps K --warmup W [--workload NAME] [--data DIR]

N > 1: one rank per GPU over RCCL -- either already under `python -m torch.distributed.run` (the driver's
form) or typed plainly, in which case this process generates the input ONCE, shares it through /dev/shm and
starts torch.distributed.run as a child (never an exec: nothing here has touched the GPU yet).  A is split
by tile rows, B replicated, every rank runs steps 1-3 on its row block; the CSR slices of C are gathered to
rank 0 in the separate `exchange` leg (the path's one exchange step).

Prints ONE JSON line on rank 0 (driver contract) with `roofline` and `cpu_baseline` objects.
"""
import argparse
import hashlib
import importlib
import json
import os
import shutil
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

HBM_PEAK_GBS = 8000.0       # MI355X spec, /opt/skills/guides/MI355X_MICROARCH.md "HBM: 8 TB/s peak (spec)"
HBM_MEASURED_GBS = 6290.0   # same guide: achievable streaming copy rate (report against both)
WATCHDOG_S = 240            # N>1: the exchange legs (never run on real xGMI here) may take this long before the line is printed without them
WORKLOADS = ["cage4", "scircuit", "webbase-1M", "mc2depi", "cage15", "webbase-1M-r2", "cage15-r2", "scircuit-r2", "mc2depi-r2"]
DUMP_ROWPTR_MAX = 1 << 21    # --dump-outputs: at most this many row-pointer values and DUMP_ENTRIES_MAX entries of C (as row, column,
DUMP_ENTRIES_MAX = 1 << 20   # value) are written, 40 MiB of float64 in all; larger outputs are sampled at seeded positions


def kernel_alg_bytes(name, d):
    """Compulsory bytes of ONE launch of a hot-path kernel, counting the intermediates it must read and write
    (DESIGN.md 'Kernels'): the companion figure `frac_kernel_bytes`; `roofline.frac` itself is on SURVEY 8(d)'s B_alg."""
    P, TC, NZ = d["npairs"], d["ntiles_c"], d["nnz_c"]
    nA, nB, TA, TB = d["nnz_a"], d["nnz_b"], d["ntiles_a"], d["ntiles_b"]
    vb = d.get("value_bytes", 8)
    table = {
        "s2_cmask_kernel": 8 * P + 32 * TA + 32 * TB + 36 * TC,
        "s2_crowcol_kernel": 36 * TC + 16 * TC + NZ,
        "s3_accumulate_kernel": 8 * P + 8 * TC + NZ + (vb * nA + 52 * TA) + (vb * nB + 84 * TB) + vb * NZ,
        # step 2: scratch (8 B/slot) + pair ids in, masks of both operands, 40 B per C tile out; then masks in, offsets + (r<<4|c) out
        "s2_tiles_kernel": 16 * P + 32 * TA + 32 * TB + 40 * TC,
        "s2_entries_kernel": 36 * TC + NZ,
        "s3_accumulate_wide_kernel": 8 * P + 8 * TC + NZ + (vb * nA + 68 * TA) + (vb * nB + 100 * TB) + vb * NZ,
    }
    table["s2_offsets_kernel"] = 6 * TC
    if name.startswith("s3_accumulate"):            # value-typed kernels carry their template arguments in the name
        if "decode" in name:                        # rows / columns read off the 32-byte C masks instead of the (r<<4|c) bytes
            return table["s3_accumulate_wide_kernel"] - NZ + 32 * TC
        name = name.split("<")[0].split("+")[0]     # (deep plans: the two step-3 launches count as one kernel)
    return table.get(name)


def kernels_sha():
    """identity of the kernel sources a PMC traffic table was taken from"""
    h = hashlib.sha256()
    for f in ("primitives.hip", "convert.hip", "step1.hip", "step2.hip", "step3.hip", "export.hip", "spgemm.hip"):
        with open(os.path.join(ROOT, "pem-spgemm_amd", "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def seeded_positions(n, k, seed):
    """k sorted positions out of range(n), the same for the same (n, k, seed); all of them when n <= k"""
    if n <= k:
        return np.arange(n)
    return np.sort(np.random.default_rng(seed).choice(n, k, replace=False))


def dump_outputs(d, rp, ci, v, row0=0, prefix="", share=1):
    """C (or this rank's rows of it) as pem_c_export_csr hands it to a caller -> d/<prefix>c_rowptr.npy and the row, column
    and value of each entry in d/<prefix>c_{row,col,val}.npy.  Whole when small, else at seeded positions; indices as float64
    (exact), values in C's own type."""
    os.makedirs(d, exist_ok=True)
    pr = seeded_positions(len(rp), DUMP_ROWPTR_MAX // share, 1)
    pe = seeded_positions(len(ci), DUMP_ENTRIES_MAX // share, 2)
    row = np.searchsorted(rp, pe, side="right") - 1 + row0
    for name, a in (("c_rowptr", rp[pr]), ("c_row", row), ("c_col", ci[pe]), ("c_val", v[pe])):
        np.save(os.path.join(d, f"{prefix}{name}.npy"), a if a.dtype.kind == "f" else a.astype(np.float64))


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)     # REPEAT=10 (reference Makefile:34)
    ap.add_argument("--warmup", type=int, default=2)     # reference WARMUP=1 (spgemm.cu:712-714)
    ap.add_argument("--workload", default="webbase-1M", choices=WORKLOADS)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the stand-in (tests only; 1.0 = BASELINE size)")
    ap.add_argument("--data", default=None, metavar="DIR",
                    help="use DIR/<workload>.mtx (the real SuiteSparse file) through pem_mm_read when it exists; else the seeded stand-in")
    ap.add_argument("--aat", action="store_true", help="C = A*A^T instead of A^2 (default for mc2depi)")
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"],
                    help="value type: f64 = the reference's ValueType and BASELINE's metric; f32 = SURVEY 8(f)-3 (not the headline)")
    ap.add_argument("--grid", default=None, metavar="RxC",
                    help="N>1: 2-D partition (SURVEY 8(f)-4), R row blocks of A x C column blocks of B, R*C = --gpus; each rank "
                         "holds only its rows of A and its columns of B.  Default: 1-D row blocks, B replicated (the BASELINE configs)")
    ap.add_argument("--chunks", type=int, default=-1, metavar="K",
                    help="N>1, 1-D: also time the pipelined form -- each rank's row block in K chunks, chunk c's CSR travelling "
                         "to rank 0 while chunk c+1 computes (SURVEY 8(f)-4); reported as exchange.pipelined.  Default -1: K chosen "
                         "from C's size (~48 MB of CSR per chunk, 2..8); 0: off")
    ap.add_argument("--no-graph", action="store_true", help="time plain stream launches instead of hipGraph replay of the repeat passes")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-r2", action="store_true", help="skip the continuity leg: the round-2 stand-in of the headline workload timed beside it")
    ap.add_argument("--no-gather", action="store_true", help="N>1: leave the C slices on their ranks")
    ap.add_argument("--no-tune-split", action="store_true", help="N>1, A^2 row blocks: keep the first cut (balanced tile-level products) "
                                                                 "instead of re-cutting it from measured per-rank times")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write the C of the last one as DIR/*.npy (a seeded sample when large; N>1: per rank)")
    ap.add_argument("--shared-input", default=None, metavar="DIR", help=argparse.SUPPRESS)   # set by the self-launcher
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


# --------------------------------------------------------------------------------------------------------------
# input: real .mtx under --data, else the seeded stand-in; produced once per job and shared between the ranks
# --------------------------------------------------------------------------------------------------------------
def produce_input(args):
    """-> (rows, cols, I, J, V, source, seconds): host-side data preparation, outside every timed region"""
    t0 = time.perf_counter()
    if args.data:
        path = os.path.join(args.data, args.workload + ".mtx")
        if os.path.exists(path):
            graft.load_package()
            hostio = importlib.import_module("pem_spgemm_amd.hostio")
            m = hostio.mm_read(path)
            return m["rows"], m["cols"], m["I"], m["J"], m["V"], "real", time.perf_counter() - t0
    graft.load_package()
    standins = importlib.import_module("pem_spgemm_amd.standins")
    rows, cols, I, J, V = standins.make(args.workload, args.scale)
    return rows, cols, I, J, V, "synthetic", time.perf_counter() - t0


def save_shared(d, rows, cols, I, J, V, source, secs):
    os.makedirs(d, exist_ok=True)
    np.save(os.path.join(d, "I.npy"), I)
    np.save(os.path.join(d, "J.npy"), J)
    np.save(os.path.join(d, "V.npy"), V)
    with open(os.path.join(d, "meta.json"), "w") as f:
        json.dump(dict(rows=int(rows), cols=int(cols), source=source, secs=secs), f)


def load_shared(d):
    meta = json.load(open(os.path.join(d, "meta.json")))
    return (meta["rows"], meta["cols"], np.load(os.path.join(d, "I.npy")), np.load(os.path.join(d, "J.npy")),
            np.load(os.path.join(d, "V.npy")), meta["source"], meta["secs"])


def shm_dir(tag):
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else (os.environ.get("TMPDIR") or "/tmp")
    return os.path.join(base, f"pem_bench_{tag}")


def self_launch(args, argv):
    """`python bench.py --gpus N` typed without a launcher: generate once, share, start N ranks as a CHILD process."""
    d = shm_dir(f"{os.getpid()}")
    try:
        save_shared(d, *produce_input(args))
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + argv + ["--shared-input", d]
        env = dict(os.environ, MASTER_ADDR="127.0.0.1")
        return subprocess.call(cmd, env=env)     # the ranks' stdout (rank 0's JSON line) passes straight through
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    args = parse_args(argv)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args, argv))

    import torch
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        if rank == 0:
            print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}", file=sys.stderr)
        sys.exit(2)
    if not torch.cuda.is_available():
        print("bench.py: no GPU visible; the product path has no CPU fallback", file=sys.stderr)
        sys.exit(3)
    # one rank per GPU; PEM_DIST_BACKEND=gloo lets several ranks rehearse the N>1 path on ONE card
    backend = os.environ.get("PEM_DIST_BACKEND", "nccl")
    dev_index = local_rank if backend == "nccl" else local_rank % torch.cuda.device_count()
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            try:
                dist.init_process_group("nccl", device_id=dev)   # "nccl" is RCCL on ROCm
            except Exception as e:                               # noqa: BLE001 -- the timed path has no collective: keep measuring
                print(f"bench.py: rank {rank}: RCCL did not come up ({type(e).__name__}: {e}); barrier and timing reductions over gloo, "
                      f"the exchange legs will report their own error", file=sys.stderr)
                backend = "gloo"
                dist.init_process_group("gloo")
        else:
            dist.init_process_group(backend)

    pkg = graft.load_package()
    mg = importlib.import_module("pem_spgemm_amd.multigpu")

    aat = args.aat or args.workload.startswith("mc2depi")
    # the input is produced once per job: by the self-launcher, or by rank 0 (shared through /dev/shm)
    made_dir = None
    if world == 1:
        rows, cols, I, J, V, source, t_gen = produce_input(args)
    else:
        d = args.shared_input
        if d is None:
            d = shm_dir(f"port{os.environ.get('MASTER_PORT', '0')}")
            if rank == 0:
                save_shared(d, *produce_input(args))
                made_dir = d
            dist.barrier()
        rows, cols, I, J, V, source, t_gen = load_shared(d)
        if made_dir is not None or args.shared_input is None:
            dist.barrier()                       # everyone has loaded: rank 0 may remove the files
            if made_dir is not None:
                shutil.rmtree(made_dir, ignore_errors=True)

    # inputs resident in HBM before anything is timed
    np_dt, torch_dt, vbytes = (np.float32, torch.float32, 4) if args.dtype == "f32" else (np.float64, torch.float64, 8)
    if args.dtype == "f32":
        V = V.astype(np.float32)
    ctx = pkg.Context(dev_index)
    grid = None
    if args.grid:
        nrb, ncb = (int(x) for x in args.grid.lower().split("x"))
        if nrb * ncb != world:
            if rank == 0:
                print(f"bench.py: --grid {args.grid} needs {nrb * ncb} ranks, got {world}", file=sys.stderr)
            sys.exit(2)
        grid = (nrb, ncb)

    def upload(mask=None, swap=False):
        a, b = (J, I) if swap else (I, J)
        if mask is not None:
            a, b, v = np.ascontiguousarray(a[mask]), np.ascontiguousarray(b[mask]), np.ascontiguousarray(V[mask])
        else:
            v = V
        t = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (a, b, v)]
        torch.cuda.synchronize()
        return t, len(a)

    split_tuning = None
    if grid is None:
        (dI, dJ, dV), nnz = upload()
        if aat:
            # B = A^T whole (replicated); A only as far as this rank multiplies it: the row block is cut from the
            # COO on the host, with boundaries balanced on the tile-level products read off B's tile CSC
            B = pkg.Tiled.from_coo_device(ctx, rows, cols, nnz, dI.data_ptr(), dJ.data_ptr(), dV.data_ptr(), True, dtype=np_dt)
            if world == 1:
                A = pkg.Tiled.from_coo_device(ctx, rows, cols, nnz, dI.data_ptr(), dJ.data_ptr(), dV.data_ptr(), False, dtype=np_dt)
                bounds = pkg.split_tile_rows(ctx, A, B, 1)
            else:
                bounds = mg.row_bounds_from_transpose(B.array("tile_rowptr"), B.array("tile_colptr"), B.array("tile_rowidx"), world)
                lo_t, hi_t = mg.slice_bounds(bounds, rank)
                (sI, sJ, sV), snz = upload(mg.restrict(I, lo_t, hi_t))
                A = pkg.Tiled.from_coo_device(ctx, rows, cols, snz, sI.data_ptr(), sJ.data_ptr(), sV.data_ptr(), False, dtype=np_dt)
                del sI, sJ, sV
        else:
            A = B = pkg.Tiled.from_coo_device(ctx, rows, cols, nnz, dI.data_ptr(), dJ.data_ptr(), dV.data_ptr(), False, dtype=np_dt)
            bounds = pkg.split_tile_rows(ctx, A, B, world)
            if world > 1 and not args.no_tune_split:
                # setup, untimed: re-cut the row blocks from measured per-rank pass times (multigpu.tune_row_bounds); any failure
                # keeps the first cut
                try:
                    first = [int(x) for x in bounds]
                    bounds, hist = mg.tune_row_bounds(pkg, ctx, A, B, bounds, rank, world, dev, graph=not args.no_graph)
                    ctx.set_graph_replay(False)
                    split_tuning = {"first_cut": first, "cut": [int(x) for x in bounds],
                                    "rounds": [{"max_ms": float(t.max()), "min_ms": float(t.min()), "mean_ms": float(t.mean())} for _, t in hist],
                                    "what": "row blocks re-cut from measured per-rank pass times before anything is timed "
                                            "(first cut: tile-level product counts, pem_split_tile_rows)"}
                except Exception as e:                          # noqa: BLE001
                    ctx.set_graph_replay(False)
                    split_tuning = {"error": f"{type(e).__name__}: {e}"}
                    bounds = pkg.split_tile_rows(ctx, A, B, world)
        del dI, dJ, dV
        lo, hi = mg.slice_bounds(bounds, rank)
        flop = pkg.flop_count(ctx, A, B)
        if world > 1 and aat:                    # every rank counted its own row block
            ft = torch.tensor([flop], dtype=torch.int64, device=dev)
            dist.all_reduce(ft)
            flop = int(ft.item())
    else:
        # rank (i, j) uploads and tiles only rows block i of A and columns block j of B
        BI, BJ = (J, I) if aat else (I, J)
        brows, bcols = (cols, rows) if aat else (rows, cols)
        rb = mg.balanced_tile_bounds(I, rows, grid[0])
        cb = mg.balanced_tile_bounds(BJ, bcols, grid[1])
        gi, gj = mg.grid_coords(rank, grid[1])
        ma, mb = mg.restrict(I, rb[gi], rb[gi + 1]), mg.restrict(BJ, cb[gj], cb[gj + 1])
        dA = [torch.from_numpy(np.ascontiguousarray(x[ma])).to(dev) for x in (I, J, V)]
        dB = [torch.from_numpy(np.ascontiguousarray(x[mb])).to(dev) for x in (BI, BJ, V)]
        torch.cuda.synchronize()
        A = pkg.Tiled.from_coo_device(ctx, rows, cols, int(ma.sum()), dA[0].data_ptr(), dA[1].data_ptr(), dA[2].data_ptr(), False, dtype=np_dt)
        B = pkg.Tiled.from_coo_device(ctx, brows, bcols, int(mb.sum()), dB[0].data_ptr(), dB[1].data_ptr(), dB[2].data_ptr(), False, dtype=np_dt)
        del dA, dB
        ft = torch.tensor([pkg.flop_count(ctx, A, B)], dtype=torch.int64, device=dev)   # every product lies in exactly one block
        dist.all_reduce(ft)
        flop = int(ft.item())
        lo, hi = rb[gi], rb[gi + 1]

    # ---- the first product on a fresh plan: allocations + the three size read-backs, what a CLI user pays once.
    # This is the reference-compatible t_total (its loop re-allocates 11 buffers and reads 3 sizes back on EVERY
    # iteration, spgemm.cu:1138-1295); measured on two fresh plans, the second one after the kernels' code objects
    # are loaded.
    cold_ms = []
    for _ in range(2):
        p0 = pkg.CPlan(ctx, A, B, lo, hi)
        ctx.synchronize()
        t0 = time.perf_counter()
        p0.spgemm()
        cold_ms.append((time.perf_counter() - t0) * 1e3)
        del p0
    plan = pkg.CPlan(ctx, A, B, lo, hi)

    gather = world > 1 and not args.no_gather
    bufs = {}

    def step():
        """the metric's unit: step1 + step2 + step3 on this rank's row block (spgemm.cu:1136-1341)"""
        plan.spgemm()

    def exchange():
        """N>1 only: tiled C slice -> CSR on the device, then gather of the slices to rank 0 over RCCL"""
        info = plan.info()
        nrows, nz = info["row_end"] - info["row_begin"], info["nnz_c"]
        if bufs.get("nz") != nz:
            bufs.update(nz=nz, rp=torch.empty(nrows + 1, dtype=torch.int32, device=dev),
                        ci=torch.empty(max(nz, 1), dtype=torch.int32, device=dev),
                        v=torch.empty(max(nz, 1), dtype=torch_dt, device=dev))
        plan.export_csr_device(bufs["rp"].data_ptr(), bufs["ci"].data_ptr(), bufs["v"].data_ptr())
        ctx.synchronize()
        if grid is None:
            bufs["out"] = mg.gather_csr_slices(bufs["rp"], bufs["ci"][:nz], bufs["v"][:nz], dst=0)
        else:
            bufs["out"] = mg.gather_csr_blocks(bufs["rp"], bufs["ci"][:nz], bufs["v"][:nz], grid[1], dst=0)

    def fence():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def timed(fn, n):
        fence()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        fence()
        el = time.perf_counter() - t0
        if dist is not None:
            te = torch.tensor([el], dtype=torch.float64, device=dev)
            dist.all_reduce(te, op=dist.ReduceOp.MAX)
            el = float(te.item())
        return el

    for _ in range(args.warmup):
        step()
    # every pass re-reading its sizes (PEM_OPT_WARM = 0): buffers re-used, three host round trips per pass
    plan.set_option("warm", 0)
    step()
    readback_ms = ctx.timings()["spgemm_wall_ms"]
    plan.set_option("warm", 1)
    step()
    step()
    tm = ctx.timings()          # step1/2/3 spans of a repeat pass launched kernel by kernel (a replayed graph has no step events)
    stream_ms = tm["spgemm_wall_ms"]
    use_graph = not args.no_graph
    if use_graph:
        ctx.set_graph_replay(True)   # the timed passes replay the captured pass as one hipGraph: same kernels, no launch gaps
        step()                       # capture + first replay, outside the timed region
    elapsed = timed(step, args.steps)
    if args.dump_outputs:
        rp, ci, v = plan.export_csr()
        dump_outputs(args.dump_outputs, rp, ci, v, row0=plan.info()["row_begin"], prefix=f"rank{rank}_" if world > 1 else "", share=world)
        del rp, ci, v
    # the same passes one by one (each ends in the library's own stream synchronisation): min / mean / max
    per_pass = []
    for _ in range(max(args.steps, 1)):
        step()
        per_pass.append(ctx.timings()["spgemm_wall_ms"])
    tm["spgemm_wall_ms"] = per_pass[-1]
    ctx.set_graph_replay(False)
    # The metric times step1+2+3 (BASELINE.json); collecting the row blocks on one GPU is the path's exchange
    # step and is timed separately over the same K passes (it is bounded by the root's xGMI ingest, not compute).
    # Nothing of the exchange runs before the metric above is in hand, and a failure in it is reported, not fatal.
    ms_per_step = elapsed * 1e3 / max(args.steps, 1)
    info = plan.info()

    # per-kernel device time, measured live with HIP events on the library's stream (separate
    # pass so the two event records per launch stay out of the timed region above)
    ctx.set_kernel_profiling(True)
    ctx.reset_kernel_stats()
    nprof = max(1, min(args.steps, 3))
    for _ in range(nprof):
        plan.spgemm()
    stats = ctx.kernel_stats()
    ctx.set_kernel_profiling(False)
    dims = dict(value_bytes=vbytes, npairs=info["npairs"], ntiles_c=info["ntiles_c"], nnz_c=info["nnz_c"], nnz_a=A.nnz, nnz_b=B.nnz,
                ntiles_a=A.ntiles, ntiles_b=B.ntiles)
    kern = {k: dict(calls_per_step=v["calls"] / nprof, avg_ms=v["total_ms"] / max(v["calls"], 1), ms_per_step=v["total_ms"] / nprof)
            for k, v in stats.items()}
    # deep plans run step 3 as TWO launches (many-pair tiles in s3_band_kernel, the rest in the entry-per-lane kernel): for the
    # roofline they are one kernel -- B_alg is a whole product's bytes -- with the sum of the two durations
    s3_pair = sorted(k for k in kern if k.startswith("s3_band_kernel") or k.endswith(",deep,band>"))
    if len(s3_pair) == 2:
        both = [kern.pop(k) for k in s3_pair]
        kern["s3_accumulate_wide_kernel+s3_band_kernel" + s3_pair[1][s3_pair[1].index("<"):]] = dict(
            calls_per_step=1.0, avg_ms=sum(b["avg_ms"] for b in both), ms_per_step=sum(b["ms_per_step"] for b in both),
            parts={k: b["ms_per_step"] for k, b in zip(s3_pair, both)})
    dom = max(kern, key=lambda k: kern[k]["ms_per_step"]) if kern else None

    # B_alg = compulsory CSR traffic of one product (this rank's slice at N>1)
    nrows_c = info["row_end"] - info["row_begin"]
    b_alg = 12 * (A.nnz + B.nnz + info["nnz_c"]) + 4 * (A.rows + 1) + 4 * (B.rows + 1) + 4 * (nrows_c + 1)
    t_kernel_ms = tm["step1_ms"] + tm["step2_ms"] + tm["step3_ms"]

    roofline = None
    if dom is not None:
        kb = kernel_alg_bytes(dom, dims)
        dur_s = kern[dom]["avg_ms"] * 1e-3
        ach = b_alg / dur_s / 1e9
        traffic, traffic_source = None, None
        tpath = os.path.join(ROOT, "profiles", "pmc_traffic.json")   # written by tools/pmc_summary.py from separate --pmc passes
        if os.path.exists(tpath) and args.workload == "webbase-1M" and args.scale == 1.0 and world == 1 and source == "synthetic":
            try:
                tj = json.load(open(tpath))
                sha = tj.get("__meta__", {}).get("kernels_sha")
                if sha == kernels_sha():             # a table taken from other kernel sources says nothing about this run
                    traffic = tj.get(dom, {}).get("hbm_bytes_per_launch")
                    traffic_source = (f"profiles/pmc_traffic.json ({tj.get('__meta__', {}).get('source', 'rocprofv3 --pmc, separate passes')}; "
                                      f"kernels sha {sha})")
                else:
                    traffic_source = f"none: profiles/pmc_traffic.json was taken from kernels sha {sha}, this run is {kernels_sha()}"
            except Exception:
                traffic = None
        roofline = dict(bound="hbm", kernel=dom, achieved=ach, peak=HBM_PEAK_GBS, unit="GB/s", frac=ach / HBM_PEAK_GBS,
                        traffic=traffic, traffic_source=traffic_source,
                        alg_bytes="SURVEY 8(d) B_alg = 12*(nnzA+nnzB+nnzC) + 4*(rowsA+rowsB+rowsC+3), the whole product's compulsory CSR bytes",
                        note="achieved/frac divide the WHOLE product's bytes by the dominant kernel's time (the contract's definition); the "
                             "pass as a whole is roofline_pipeline.frac (B_alg / ms_per_step, also copied here as pipeline_frac), and the "
                             "kernel on its own compulsory bytes is frac_kernel_bytes",
                        pipeline_frac=b_alg / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS,
                        alg_bytes_per_launch=b_alg, avg_launch_ms=kern[dom]["avg_ms"], launches_per_step=kern[dom]["calls_per_step"],
                        frac_vs_measured_peak=ach / HBM_MEASURED_GBS,
                        kernel_bytes_per_launch=kb, frac_kernel_bytes=(kb / dur_s / 1e9 / HBM_PEAK_GBS) if kb else None)

    total_nnz_c, total_tc, total_p = info["nnz_c"], info["ntiles_c"], info["npairs"]
    if dist is not None:
        tt = torch.tensor([info["nnz_c"], info["ntiles_c"], info["npairs"]], dtype=torch.int64, device=dev)
        dist.all_reduce(tt)
        total_nnz_c, total_tc, total_p = [int(x) for x in tt.tolist()]

    # --- from here on: the exchange legs (N>1) and the single-GPU extras; the metric, the step spans, the kernel table and the
    # roofline above are complete, so a leg that hangs on hardware it has never run on (this pool hands out one-GPU boxes)
    # cannot take the headline line with it: a watchdog prints the line without the leg and ends the process
    import threading
    emitted = threading.Event()
    state = {"exchange": None, "export": None, "conversion": None, "standin_r2": None, "cpu_baseline": None}

    def emit():
        """rank 0 prints the ONE JSON line (once)"""
        if emitted.is_set():
            return
        emitted.set()
        if rank != 0:
            return
        gf = lambda ms: 2.0 * flop / (ms * 1e-3) / 1e9    # noqa: E731
        out = {
            "metric": "SpGEMM GFLOP/s (2*flop / t(step1+step2+step3))",
            "value": gf(ms_per_step),
            "unit": "GFLOP/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "cold_value": gf(cold_ms[-1]),     # the reference's own accounting: first pass on a fresh plan, allocations + size read-backs (see t_total)
            "cold_ms": cold_ms[-1],
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": args.dtype,
            "data": source,
            "config": {"workload": (f"{args.workload} (real file under --data)" if source == "real" else
                                    f"{args.workload} stand-in (seeded synthetic, scale {args.scale}; host/standin.cpp, product calibrated "
                                    f"to the literature in round 3)" if not args.workload.endswith("-r2") else
                                    f"{args.workload} (round-2 numpy stand-in, scale {args.scale})") + (" A*A^T" if aat else " A^2"),
                       "rows": rows, "cols": cols, "nnz": int(len(I)), "flop": int(flop), "C_nnz": total_nnz_c, "C_tiles": total_tc,
                       "tile_pairs": total_p, "A_tiles": int(A.ntiles) if not (aat and world > 1) else None,
                       "compression_ratio": flop / max(total_nnz_c, 1),
                       "parallelism": (f"rowblock{world}" if grid is None else f"grid{grid[0]}x{grid[1]}") + ("+gather" if gather else "")},
            "roofline": roofline,
            "roofline_pipeline": {"bound": "hbm", "B_alg_bytes": b_alg, "t_kernel_ms": t_kernel_ms, "t_step_ms": ms_per_step,
                                  "achieved": b_alg / (ms_per_step * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                  "frac": b_alg / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                  "frac_vs_measured_peak": b_alg / (ms_per_step * 1e-3) / 1e9 / HBM_MEASURED_GBS,
                                  "frac_kernel_spans": b_alg / (t_kernel_ms * 1e-3) / 1e9 / HBM_PEAK_GBS if t_kernel_ms > 0 else None,
                                  "note": "rank 0 slice: B_alg over the timed pass (ms_per_step) and over the hipEvent spans of step1+2+3"},
            "t_total": {"cold_ms": cold_ms[-1], "cold_first_ms": cold_ms[0], "cold_value": gf(cold_ms[-1]),
                        "readback_ms": readback_ms, "stream_ms": stream_ms,
                        "min_ms": min(per_pass), "mean_ms": sum(per_pass) / len(per_pass), "max_ms": max(per_pass), "min_value": gf(min(per_pass)),
                        "note": "cold = first pem_spgemm on a fresh plan (every device allocation + 3 size read-backs: the reference's "
                                "per-iteration cost, spgemm.cu:1136-1341; cold_first also loads the code objects); readback = buffers "
                                "re-used, sizes read back every pass (PEM_OPT_WARM = 0); stream = warm plan, plain launches; min/mean/max = "
                                "the timed passes one by one (this rank)"},
            "cpu_baseline": state["cpu_baseline"],
            "exchange": state["exchange"],
            "steps_ms": {"step1": tm["step1_ms"], "step2": tm["step2_ms"], "step3": tm["step3_ms"], "wall_last": tm["spgemm_wall_ms"],
                         "note": "step spans: one repeat pass launched kernel by kernel before the timed region; timed passes: "
                                 + ("hipGraph replay of that pass" if use_graph else "the same, no graph")},
            "launch": "hipgraph" if use_graph else "stream",
            "note": "value = warm-plan passes (all kernels of step1+2+3 run every pass; buffers and sizes are kept from the plan's "
                    "first pass, device-verified) replayed as one hipGraph; the first-product cost is t_total.cold_ms.  Reference "
                    "arrays with no reader on this path (Ctiles_rowPtr, _C_tileRowIdx; Ctiles_rowColIdx on plans whose step 3 reads the "
                    "C masks) are materialised on demand, outside the pass.",
            "conversion_ms": {"A": A.conv_ms, "A_tile_kernels": A.conv_tile_kernel_ms},
            "conversion": state["conversion"],
            "export": state["export"],
            "standin_r2": state["standin_r2"],
            "split_tuning": split_tuning,
            "memory": ctx.memory_stats(),
            "kernels": kern,
            "gen_s": t_gen,
        }
        print(json.dumps(out), flush=True)
    watchdog = None
    if world > 1:
        def bail():
            if emitted.is_set():
                return
            state["exchange"] = {"error": "the exchange legs did not finish within %d s (leg in flight: %s); metric and roofline above are complete"
                                          % (WATCHDOG_S, state.get("leg", "?"))}
            emit()
            os._exit(3)                                           # a hung exchange is a failed run: the launcher and the driver must see it
        watchdog = threading.Timer(WATCHDOG_S, bail)
        watchdog.daemon = True
        watchdog.start()

    exchange_ms, exchange_error = None, None
    if gather:
        try:
            state["leg"] = "sequential gather"
            exchange()                                            # warm: communicators, receive buffers
            exchange_ms = timed(exchange, args.steps) * 1e3 / max(args.steps, 1)
        except Exception as e:                                    # noqa: BLE001 -- keep the headline line
            exchange_error = f"{type(e).__name__}: {e}"
            gather = False
    pipelined = None
    nchunks = args.chunks
    if nchunks < 0 and world > 1:
        # the overlapped gather is part of the default N>1 line: K from the bytes one rank sends (12 B per C entry)
        tn = torch.tensor([plan.info()["nnz_c"]], dtype=torch.int64, device=dev)
        if dist is not None:
            dist.all_reduce(tn, op=dist.ReduceOp.MAX)
        nchunks = int(max(2, min(8, -(-int(tn.item()) * (vbytes + 4) // (48 << 20)))))
    if gather and grid is None and nchunks > 0 and not aat:
      try:
          cb = pkg.split_tile_rows(ctx, A, B, world * nchunks)
          state["leg"] = "pipelined gather"
          crb = mg.ChunkedRowBlock(pkg, ctx, A, B, cb, rank, nchunks, torch_dt, dst=0)
          crb.run_pass()                                            # sizes + staging buffers; plans warm up
          crb.run_pass()
          t_pipe = timed(lambda: bufs.__setitem__("pipe_out", crb.run_pass()), args.steps) * 1e3 / max(args.steps, 1)
          pipelined = {"chunks": nchunks, "ms_per_step": t_pipe,
                       "what": "steps 1-3 of every chunk + device CSR export + gather to rank 0, chunk c in flight while chunk c+1 computes",
                       "sequential_ms_per_step": ms_per_step + exchange_ms,
                       "value_with_exchange": 2.0 * flop / (t_pipe * 1e-3) / 1e9}
          if rank == 0:
              prp, pci, pv = bufs["pipe_out"]
              pipelined["fingerprint"] = {"nnz": int(pci.numel()), "colidx_sum": int(pci.to(torch.int64).sum().item()),
                                          "rowptr_sum": int(prp.to(torch.int64).sum().item()),
                                          "vals_sum": float(pv.to(torch.float64).cpu().sum().item())}
      except Exception as e:                                      # noqa: BLE001 -- keep the headline line
        pipelined = {"error": f"{type(e).__name__}: {e}"}
    gathered = None
    if gather and rank == 0 and bufs.get("out") is not None:
        # fingerprint of the assembled C on the root (tests compare it across partitionings; equal arrays give equal sums)
        grp, gci, gv = bufs["out"]
        gathered = {"rows": int(grp.numel() - 1), "nnz": int(gci.numel()), "rowptr_last": int(grp[-1].item()) if grp.numel() else 0,
                    "colidx_sum": int(gci.to(torch.int64).sum().item()), "rowptr_sum": int(grp.to(torch.int64).sum().item()),
                    "vals_sum": float(gv.to(torch.float64).cpu().sum().item()), "vals_abs_sum": float(gv.to(torch.float64).abs().cpu().sum().item())}

    # a14: tiled C -> CSR on the device (what every N>1 run and every --out pays after the metric's steps); its own bytes
    export = None
    if world == 1 and info["nnz_c"] > 0:
        nrows_e, nz_e = info["row_end"] - info["row_begin"], info["nnz_c"]
        erp = torch.empty(nrows_e + 1, dtype=torch.int32, device=dev)
        eci = torch.empty(nz_e, dtype=torch.int32, device=dev)
        ev = torch.empty(nz_e, dtype=torch_dt, device=dev)
        for _ in range(2):
            plan.export_csr_device(erp.data_ptr(), eci.data_ptr(), ev.data_ptr())
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(max(args.steps, 1)):
            plan.export_csr_device(erp.data_ptr(), eci.data_ptr(), ev.data_ptr())
        ctx.synchronize()
        ex_ms = (time.perf_counter() - t0) * 1e3 / max(args.steps, 1)
        ex_bytes = (vbytes + 1) * nz_e + 8 * info["ntiles_c"] + (vbytes + 4) * nz_e + 4 * nrows_e
        export = {"ms": ex_ms, "bytes": ex_bytes, "achieved": ex_bytes / (ex_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                  "frac": ex_bytes / (ex_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                  "what": "pem_c_export_csr_device (spgemm.cu:663-695, 1493-1519 without the 16-byte-record sort); bytes = "
                          "(vals + 1 mask byte)*nnz + 8*T_C in, (vals + colidx)*nnz + 4*rows out; wall over the same K calls"}
        del erp, eci, ev

    # continuity: round 3 recalibrated the webbase-1M stand-in (its product now compresses 1.36x like the real matrix's, the
    # round-2 one 1.02x); the round-2 stand-in is timed beside it for one round so the numbers of the two rounds connect
    r2 = None
    if world == 1 and args.workload == "webbase-1M" and args.scale == 1.0 and source == "synthetic" and not args.no_r2 and not aat:
        standins_mod = importlib.import_module("pem_spgemm_amd.standins")
        r_rows, r_cols, rI, rJ, rV = standins_mod.make("webbase-1M-r2")
        if args.dtype == "f32":
            rV = rV.astype(np.float32)
        rt = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (rI, rJ, rV)]
        torch.cuda.synchronize()
        rA = pkg.Tiled.from_coo_device(ctx, r_rows, r_cols, len(rI), rt[0].data_ptr(), rt[1].data_ptr(), rt[2].data_ptr(), False, dtype=np_dt)
        del rt
        r_flop = pkg.flop_count(ctx, rA, rA)
        rplan = pkg.CPlan(ctx, rA, rA)
        for _ in range(3):
            rplan.spgemm()
        r_tm = ctx.timings()
        ctx.set_graph_replay(use_graph)
        rplan.spgemm()
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(max(args.steps, 1)):
            rplan.spgemm()
        ctx.synchronize()
        r_ms = (time.perf_counter() - t0) * 1e3 / max(args.steps, 1)
        ctx.set_graph_replay(False)
        ri = rplan.info()
        r_balg = 12 * (2 * rA.nnz + ri["nnz_c"]) + 4 * 3 * (r_rows + 1)
        r2 = {"workload": "webbase-1M-r2 (the round-1/2 stand-in, numpy seed 1000) A^2", "ms_per_step": r_ms, "value": 2.0 * r_flop / (r_ms * 1e-3) / 1e9,
              "flop": int(r_flop), "C_nnz": ri["nnz_c"], "C_tiles": ri["ntiles_c"], "tile_pairs": ri["npairs"], "compression_ratio": r_flop / max(ri["nnz_c"], 1),
              "steps_ms": {"step1": r_tm["step1_ms"], "step2": r_tm["step2_ms"], "step3": r_tm["step3_ms"]},
              "pipeline_frac": r_balg / (r_ms * 1e-3) / 1e9 / HBM_PEAK_GBS}
        rplan.close()
        rA.close()
        del rI, rJ, rV

    # a2-a7 again, now that the arena holds the memory (the first conversion above paid the driver allocations): COO
    # triplets resident in HBM -> tiled form; B_conv = 25*nnz + 48*T
    conversion = None
    if world == 1 and grid is None:
        (cI, cJ, cV), cn = upload()
        conv = []
        for _ in range(3):
            ctx.synchronize()
            t0 = time.perf_counter()
            Tc = pkg.Tiled.from_coo_device(ctx, rows, cols, cn, cI.data_ptr(), cJ.data_ptr(), cV.data_ptr(), False, dtype=np_dt)
            conv.append(((time.perf_counter() - t0) * 1e3, Tc.conv_ms, Tc.conv_tile_kernel_ms))
            nt_c = Tc.ntiles
            Tc.close()
        del cI, cJ, cV
        b_conv = (8 + 2 * vbytes + 1) * cn + 48 * nt_c
        best = min(c[0] for c in conv)
        conversion = {"first_ms": A.conv_ms, "ms": best, "all_ms": [c[0] for c in conv], "bytes": b_conv,
                      "achieved": b_conv / (best * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": b_conv / (best * 1e-3) / 1e9 / HBM_PEAK_GBS,
                      "what": "pem_tiled_from_coo_device wall (COO already in HBM; two size read-backs inside); first_ms = the first "
                              "conversion on the fresh context (driver allocations), ms = best of three with the arena warm; "
                              "B_conv = SURVEY 8(d): 16*nnz COO in (two int32 + one fp64) + 9*nnz + 48*T tiled out"}

    cpu_baseline = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        # CPU port (oracle/ref_serial_csr.c: the reference has no CPU SpGEMM path) on this box's
        # host cores -- a reported baseline beside the GPU number, never the thing measured above.
        o = graft.load_oracle()
        threads = o.max_threads()
        oa = o.Csr(rows, cols, I, J, V, False)
        ob = o.Csr(rows, cols, I, J, V, True) if aat else oa
        # the reference's policy for its own timed loop (spgemm.cu:712-718, Makefile:34) -- WARMUP 1, then REPEAT
        # passes, mean and min -- with REPEAT bounded so the default line stays within a couple of seconds of CPU work
        CPU_WARMUP, CPU_REPEAT = 1, (5 if flop <= 400_000_000 else 1)
        runs = []
        for it in range(CPU_WARMUP + CPU_REPEAT):
            t1 = time.perf_counter()
            oc = o.csr_spgemm(oa, ob, threads)
            runs.append(time.perf_counter() - t1)
            assert oc.nnz == total_nnz_c, f"CPU port C nnz {oc.nnz} != GPU {total_nnz_c}"
            del oc
        timed_runs = runs[CPU_WARMUP:] if len(runs) > CPU_WARMUP else runs
        tc, tc_min = sum(timed_runs) / len(timed_runs), min(timed_runs)
        serial_ms = None
        if flop <= 400_000_000:                  # bounded: the serial pass of the headline workload takes about a second
            t1 = time.perf_counter()
            o.csr_spgemm(oa, ob, 1)
            serial_ms = (time.perf_counter() - t1) * 1e3
        cpu_baseline = dict(value=2.0 * flop / tc / 1e9, unit="GFLOP/s", cores=threads, kind="port",
                            sample=f"full {args.workload} {'file' if source == 'real' else 'stand-in'}: OpenMP row-parallel Gustavson CSR port, "
                                   f"warm-up {CPU_WARMUP} + {len(timed_runs)} timed runs (mean {tc * 1e3:.0f} ms, min {tc_min * 1e3:.0f} ms); 1 run on one core",
                            ms=tc * 1e3, min_ms=tc_min * 1e3, min_value=2.0 * flop / tc_min / 1e9, runs_ms=[r * 1e3 for r in runs], warmup=CPU_WARMUP,
                            repeat=len(timed_runs), serial_ms=serial_ms,
                            serial_value=(2.0 * flop / (serial_ms * 1e-3) / 1e9) if serial_ms else None)

    state["exchange"] = ({"error": exchange_error} if exchange_error else None) if exchange_ms is None else {
        "ms_per_step": exchange_ms, "what": "pem_c_export_csr_device + gather of the CSR row blocks to rank 0 (P2P over RCCL)",
        "bytes_to_root": 12 * (total_nnz_c - info["nnz_c"]),
        "value_with_exchange": 2.0 * flop / ((ms_per_step + exchange_ms) * 1e-3) / 1e9,
        "gathered": gathered, "pipelined": pipelined}
    state.update(export=export, conversion=conversion, standin_r2=r2, cpu_baseline=cpu_baseline)
    if watchdog is not None:
        watchdog.cancel()
    emit()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
