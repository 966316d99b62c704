"""Frontier products and breadth-first search on the device (pem_tiled_mxv_frontier / pem_tiled_bfs) against dense pem_tiled_mxv.

    python tools/frontier_pass.py [--passes 10] [--warmup 2] [--only webbase-1M-r2,cage15] [--out result.json]

Per workload (seeded stand-ins, fp64), medians over --passes after --warmup of the call's host clock (launch to a context
synchronise) and of its kernels' device time (the library's per-kernel events: pack + mark + walk; the flag memset is not a kernel
and shows in the host clock only):
  dense     all x present, no mask, under plus_times, lor_land and plus_pair, both orientations: pem_tiled_mxv (unchanged by the
            frontier work, so the parent's number), the frontier call with x_present = None (the walk alone) and with an all-ones
            x_present (pack and mark as well); ratios to mxv.
  presence  present fractions 1, 1/16, 1/256, 1/4096 and a single index, scattered (independent draws) and clustered (whole
            16-entry segments), plus_times, both orientations: time, the share of lines flagged (read back through the test hook)
            and the share of entries live.  crossover: the largest fraction at which the frontier call's kernel time is below mxv's.
  mask      allowed fractions 1/2, 1/16, 1/256 (independent draws), all x present.
  bfs       from the highest-degree vertex: pem_tiled_bfs (median host clock, it waits), the same search as a torch loop over
            mxv_frontier with every level clocked (level time and frontier size), and the route the parent commit offers: a torch loop
            over dense mxv(lor_land, transpose) with the visited filter in torch.
Bytes: the compulsory traffic of one frontier call as a fraction of 8 TB/s over the kernels' device time.  The compulsory set:
  the presence bytes (nx) and the mask bytes (ny) read once; the words written and the nonzero ones' segment pointers and tile lists
  read by mark (2 bytes per segment twice, 8 bytes per nonzero segment, 4 per tile of such a segment); one flag byte per line written
  and read; per flagged line with an allowed output its two line pointers (8 bytes); per tile of such a line its offset, minor index
  (and, for columns, base) and word (10 or 14 bytes); the 1-byte (major, minor) of every entry in a tile with a nonzero word; value
  and x (2 x 8 bytes; none under plus_pair) of every live entry; y written where allowed (8 bytes; with accumulate only where a term
  arrived) and out_present (ny) when asked for.  What the dense call must move in addition is every other entry's byte, value and x.
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
import frontierref as fr  # noqa: E402

DEFAULT = ("webbase-1M-r2", "cage15")
FRACTIONS = (("1", 1.0), ("1/16", 1 / 16), ("1/256", 1 / 256), ("1/4096", 1 / 4096), ("one", 0.0))


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
    ts = []
    for _ in range(passes):
        ctx.reset_kernel_stats()
        ctx.set_kernel_profiling(True)
        fn()
        ctx.synchronize()
        ctx.set_kernel_profiling(False)
        ts.append(sum(v["total_ms"] for v in ctx.kernel_stats().values()))
    return statistics.median(ts)


def _timed(ctx, fn, passes, warmup):
    fn()
    return dict(kernel_ms=round(_kernel_ms(ctx, fn, passes), 4), wall_ms=round(_median(fn, ctx, passes, warmup), 4))


def _frac(nbytes, ms):
    return round(nbytes / (ms * 1e-3) / 8.0e12, 4) if ms > 0 else 0.0


class Shape:
    """the host view of one orientation: per entry its line, its x index and its tile; per tile its line and segment"""

    def __init__(self, M, I, J, col):
        self.col = col
        self.nx, self.ny = (M.rows, M.cols) if col else (M.cols, M.rows)
        self.major, self.minor = (J, I) if col else (I, J)
        self.nlines, self.nseg = (self.ny + 15) // 16, (self.nx + 15) // 16
        key = (self.major // 16).astype(np.int64) * self.nseg + self.minor // 16
        tiles, self.entry_tile = np.unique(key, return_inverse=True)
        self.tile_line, self.tile_seg = tiles // self.nseg, tiles % self.nseg
        self.nnz = len(I)

    def shares_and_bytes(self, present, allowed, semiring, accumulate=False, want_present=False, vb=8):
        word_on = np.zeros(self.nseg, bool)
        if present is None:
            word_on[:] = True
        else:
            np.logical_or.at(word_on, np.arange(self.nx) // 16, present)
        tile_on = word_on[self.tile_seg]
        flag = np.zeros(self.nlines, bool)
        flag[self.tile_line[tile_on]] = True
        line_ok = flag.copy()
        if allowed is not None:
            any_allowed = np.zeros(self.nlines, bool)
            np.logical_or.at(any_allowed, np.arange(self.ny) // 16, allowed)
            line_ok &= any_allowed
        live = tile_on[self.entry_tile] & line_ok[self.major // 16]
        byte_read = int(live.sum())
        if present is not None:
            live &= present[self.minor]
        if allowed is not None:
            live &= allowed[self.major]
        nlive = int(live.sum())
        walked_tiles = int(line_ok[self.tile_line].sum())
        b = 0
        if present is not None:
            b += self.nx + 4 * self.nseg + 8 * int(word_on.sum()) + 4 * int(tile_on.sum()) + 2 * self.nlines
        if allowed is not None:
            b += self.ny
        b += 8 * int(line_ok.sum()) + walked_tiles * (14 if self.col else 10) + byte_read
        b += nlive * (0 if semiring == "plus_pair" else 2 * vb)
        nallowed = self.ny if allowed is None else int(allowed.sum())
        b += vb * (len(np.unique(self.major[live])) if accumulate else nallowed)
        if want_present:
            b += self.ny
        return dict(flagged_line_share=round(float(flag.mean()), 6), live_entry_share=round(nlive / max(self.nnz, 1), 6), bytes=int(b))


def _present(kind, frac, n, rng):
    p = np.zeros(n, bool)
    if frac >= 1.0:
        p[:] = True
    elif frac == 0.0:
        p[n // 2] = True
    elif kind == "scattered":
        p = rng.random(n) < frac
    else:
        nseg = (n + 15) // 16
        p = np.repeat(rng.random(nseg) < frac, 16)[:n]
    return p


def bfs_runs(pkg, torch, ctx, M, rp, ci, passes, warmup):
    n = M.rows
    src = int(np.argmax(np.diff(rp)))
    want, wdepth, wreached = fr.bfs(n, rp, ci, src)
    lv, depth, reached = M.bfs(src)
    torch.cuda.synchronize()
    r = dict(source=src, depth=depth, reached=reached, equal=bool(np.array_equal(lv.cpu().numpy(), want)) and (depth, reached) == (wdepth, wreached))
    r["pem_tiled_bfs_wall_ms"] = round(_median(lambda: M.bfs(src), ctx, passes, warmup), 4)
    few = max(1, min(passes, 3)) if depth > 200 else passes

    def frontier_loop(levels=None):
        level = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        level[src] = 0
        visited = torch.zeros(n, dtype=torch.bool, device="cuda")
        visited[src] = True
        frontier, nxt = visited.clone(), torch.zeros(n, dtype=torch.bool, device="cuda")
        count = torch.zeros(n, dtype=torch.float64, device="cuda")
        d = 0
        while True:
            t0 = time.perf_counter()
            M.mxv_frontier(None, frontier, visited, True, "plus_pair", True, out=count, accumulate=True, out_present=nxt)
            size = int(nxt.sum())
            if levels is not None:
                levels.append(dict(level=d + 1, frontier_in=int(frontier.sum()), found=size, wall_ms=round((time.perf_counter() - t0) * 1e3, 4)))
            if not size:
                return level
            d += 1
            level[nxt] = d
            visited |= nxt
            frontier, nxt = nxt, frontier

    def dense_loop():
        level = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        level[src] = 0
        visited = torch.zeros(n, dtype=torch.bool, device="cuda")
        visited[src] = True
        x = visited.to(torch.float64)
        y = torch.empty(n, dtype=torch.float64, device="cuda")
        d = 0
        while True:
            M.mxv(x, "lor_land", transpose=True, out=y)
            nxt = (y != 0) & ~visited
            if not bool(nxt.any()):
                return level
            d += 1
            level[nxt] = d
            visited |= nxt
            x = nxt.to(torch.float64)

    levels = []
    got = frontier_loop(levels)
    r["torch_frontier_loop_equal"] = bool(np.array_equal(got.cpu().numpy(), want))
    r["torch_dense_loop_equal"] = bool(np.array_equal(dense_loop().cpu().numpy(), want))
    r["levels"] = levels
    r["torch_frontier_loop_wall_ms"] = round(_median(frontier_loop, ctx, few, 1), 4)
    r["torch_dense_mxv_loop_wall_ms"] = round(_median(dense_loop, ctx, few, 1), 4)
    r["dense_loop_over_pem_tiled_bfs"] = round(r["torch_dense_mxv_loop_wall_ms"] / r["pem_tiled_bfs_wall_ms"], 2)
    return r


def one_matrix(pkg, torch, ctx, M, passes, warmup):
    rp, ci, v = M.export_csr()
    I = np.repeat(np.arange(M.rows, dtype=np.int64), np.diff(rp))
    J = ci.astype(np.int64)
    r = dict(rows=M.rows, cols=M.cols, nnz=M.nnz, ntiles=M.ntiles)
    rng = np.random.default_rng(5)
    shapes = {col: Shape(M, I, J, col) for col in (False, True)}
    dx = {col: torch.from_numpy(rng.standard_normal(shapes[col].nx)).cuda() for col in (False, True)}
    ys = {col: torch.empty(shapes[col].ny, dtype=torch.float64, device="cuda") for col in (False, True)}
    yref = {col: torch.empty(shapes[col].ny, dtype=torch.float64, device="cuda") for col in (False, True)}
    dense, base = {}, {}
    for col in (False, True):
        o = "cols" if col else "rows"
        ones = torch.ones(shapes[col].nx, dtype=torch.bool, device="cuda")
        for s in ("plus_times", "lor_land", "plus_pair"):
            a = _timed(ctx, lambda: M.mxv(dx[col], s, transpose=col, out=yref[col]), passes, warmup)
            b = _timed(ctx, lambda: M.mxv_frontier(dx[col], semiring=s, transpose=col, out=ys[col]), passes, warmup)
            same = bool(torch.equal(ys[col].view(torch.int64), yref[col].view(torch.int64)))
            c = _timed(ctx, lambda: M.mxv_frontier(dx[col], ones, semiring=s, transpose=col, out=ys[col]), passes, warmup)
            same = same and bool(torch.equal(ys[col].view(torch.int64), yref[col].view(torch.int64)))
            nb = shapes[col].shares_and_bytes(None, None, s)["bytes"]
            dense[f"{s}_{o}"] = dict(mxv=a, frontier_all=b, frontier_ones=c, equal=same, bytes=nb, hbm_frac_frontier_all=_frac(nb, b["kernel_ms"]),
                                     kernel_ratio_all=round(b["kernel_ms"] / a["kernel_ms"], 3), wall_ratio_all=round(b["wall_ms"] / a["wall_ms"], 3),
                                     kernel_ratio_ones=round(c["kernel_ms"] / a["kernel_ms"], 3), wall_ratio_ones=round(c["wall_ms"] / a["wall_ms"], 3))
            if s == "plus_times":
                base[col] = a
    r["dense"] = dense
    presence, crossover = {}, {}
    for col in (False, True):
        o = "cols" if col else "rows"
        sh = shapes[col]
        for kind in ("scattered", "clustered"):
            best = None
            for label, frac in FRACTIONS:
                p = _present(kind, frac, sh.nx, rng)
                dp = torch.from_numpy(p).cuda()
                t = _timed(ctx, lambda: M.mxv_frontier(dx[col], dp, semiring="plus_times", transpose=col, out=ys[col]), passes, warmup)
                flags = M.frontier_line_flags(col)
                t.update(sh.shares_and_bytes(p, None, "plus_times"))
                t["flagged_line_share_device"] = round(float(flags.mean()), 6)
                t["hbm_frac"] = _frac(t["bytes"], t["kernel_ms"])
                t["kernel_ratio_to_mxv"] = round(t["kernel_ms"] / base[col]["kernel_ms"], 3)
                t["wall_ratio_to_mxv"] = round(t["wall_ms"] / base[col]["wall_ms"], 3)
                presence[f"{o}_{kind}_{label}"] = t
                if best is None and t["kernel_ms"] < base[col]["kernel_ms"]:
                    best = label
            crossover[f"{o}_{kind}"] = best
    r["presence"], r["crossover_fraction"] = presence, crossover
    masks = {}
    for col in (False, True):
        o = "cols" if col else "rows"
        sh = shapes[col]
        for label, frac in (("1/2", 0.5), ("1/16", 1 / 16), ("1/256", 1 / 256)):
            m = rng.random(sh.ny) < frac
            dm = torch.from_numpy(m).cuda()
            t = _timed(ctx, lambda: M.mxv_frontier(dx[col], None, dm, semiring="plus_times", transpose=col, out=ys[col]), passes, warmup)
            t.update(sh.shares_and_bytes(None, m, "plus_times"))
            t["hbm_frac"] = _frac(t["bytes"], t["kernel_ms"])
            t["kernel_ratio_to_mxv"] = round(t["kernel_ms"] / base[col]["kernel_ms"], 3)
            masks[f"{o}_{label}"] = t
    r["mask"] = masks
    if M.rows == M.cols:
        r["bfs"] = bfs_runs(pkg, torch, ctx, M, rp.astype(np.int64), J, passes, warmup)
    return r


def report(name, r):
    out = [f"{name}: {r['rows']} x {r['cols']}, nnz {r['nnz']}, tiles {r['ntiles']}"]
    out.append("  dense (all present, no mask): kernel ms (wall ms)          mxv | frontier, x_present=None | frontier, all-ones x_present")
    for k, d in r["dense"].items():
        out.append(f"    {k:>16}  {d['mxv']['kernel_ms']:.4f} ({d['mxv']['wall_ms']:.4f}) | {d['frontier_all']['kernel_ms']:.4f} ({d['frontier_all']['wall_ms']:.4f})"
                   f" x{d['kernel_ratio_all']:.3f} | {d['frontier_ones']['kernel_ms']:.4f} ({d['frontier_ones']['wall_ms']:.4f}) x{d['kernel_ratio_ones']:.3f}"
                   f" | equal {d['equal']} | {d['hbm_frac_frontier_all']:.3f} of 8 TB/s")
    out.append("  presence sweep (plus_times): kernel ms (wall ms), ratio to mxv kernel, lines flagged, entries live, share of 8 TB/s on the compulsory bytes")
    for k, t in r["presence"].items():
        out.append(f"    {k:>24}  {t['kernel_ms']:.4f} ({t['wall_ms']:.4f}) x{t['kernel_ratio_to_mxv']:.3f}  flagged {t['flagged_line_share']:.4f}"
                   f" (device {t['flagged_line_share_device']:.4f})  live {t['live_entry_share']:.6f}  {t['hbm_frac']:.3f}")
    out.append(f"  crossover (largest fraction below mxv's kernel time): {r['crossover_fraction']}")
    out.append("  mask sweep (all x present, plus_times): kernel ms (wall ms), ratio to mxv kernel, entries live")
    for k, t in r["mask"].items():
        out.append(f"    {k:>12}  {t['kernel_ms']:.4f} ({t['wall_ms']:.4f}) x{t['kernel_ratio_to_mxv']:.3f}  live {t['live_entry_share']:.6f}  {t['hbm_frac']:.3f}")
    if "bfs" in r:
        b = r["bfs"]
        out.append(f"  bfs from {b['source']}: depth {b['depth']}, reached {b['reached']}, equal to the host model {b['equal']}"
                   f" (torch loops {b['torch_frontier_loop_equal']}, {b['torch_dense_loop_equal']})")
        out.append(f"    pem_tiled_bfs {b['pem_tiled_bfs_wall_ms']:.3f} ms | torch loop over mxv_frontier {b['torch_frontier_loop_wall_ms']:.3f} ms | torch loop over dense "
                   f"mxv(lor_land) {b['torch_dense_mxv_loop_wall_ms']:.3f} ms = x{b['dense_loop_over_pem_tiled_bfs']:.2f} of pem_tiled_bfs")
        lv = b["levels"]
        shown = lv if len(lv) <= 40 else lv[:20] + lv[-20:]
        out.append("    level: frontier in -> found, wall ms (torch loop over mxv_frontier, one sync per level)" + ("" if len(lv) <= 40 else f" [first and last 20 of {len(lv)}]"))
        out.append("    " + "  ".join(f"{x['level']}: {x['frontier_in']}->{x['found']} {x['wall_ms']:.3f}" for x in shown))
    return "\n".join(out)


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
    results = {"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "passes": a.passes, "warmup": a.warmup}
    for name in names:
        rows, cols, I, J, V = standins.make(name, 1.0)
        A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
        results[name] = one_matrix(pkg, torch, ctx, A, a.passes, a.warmup)
        print(report(name, results[name]), flush=True)
        A.close()
        if a.out:
            with open(a.out, "w") as f:
                json.dump(results, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
