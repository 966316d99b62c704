#!/usr/bin/env python3
"""Replay one program of the sequence test (tests/test_gpu_seq.py) with per-step output.

    python tools/seq_replay.py --seed 107 [--steps 120] [--context session|torch_stream|graph_replay]
    python tools/seq_replay.py --seed 1203            (a seed from seqgen.SET2_FROM on draws from the second operation set,
                                                       one from seqgen.SET3_FROM on from the third)
    python tools/seq_replay.py --program failing.txt [--context ...]

--program reads the text a failing test printed (one JSON record per line; other lines are ignored), --seed regenerates the
program.  The program runs ONCE through the runner of tests/seqrun.py, printing every step and the model's verdict.  On a
mismatch the tool prints it and then the dependency closure of the failing step: the earlier steps that created or wrote any
handle the failing step reads, transitively (for an audit: of every live handle) -- the candidate for the reduced program.  It
never re-runs anything by itself, and a HIP error status (PEM_E_HIP) ends the run at once.
"""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def handles(rec):
    """(read, written) handle ids of a record"""
    op, ids, a = rec
    read = {h for h in ids if h is not None}
    wrote = {a["out"]} if "out" in a else set()
    if op.startswith("set_values") or op in ("step1", "step2", "step3", "spgemm", "set_semiring", "set_option"):
        wrote.add(ids[0])
    if op in ("trsv", "trsv_info", "lu_solve"):   # (the first of them builds the triangle's schedule, which stays with the tiling)
        wrote.add(ids[0])
    if op == "amg_refresh" or (op in ("colour", "colour_order", "components", "mis", "aggregate", "amg_create") and not a.get("symmetric")):
        wrote.add(ids[0])                         # (a refresh rewrites its hierarchy; symmetric = 0 may build the column schedule)
    return read, wrote


def closure(prog, step, live=None):
    """indices of the steps that created or wrote a handle step `step` reads (live: every handle, for an audit), transitively"""
    operands = {r[2]["out"]: {h for h in r[1] if h is not None} for r in prog[:step + 1]
                if r[0] in ("plan_create", "krylov_create", "amg_create") and "out" in r[2]}
    # (a derived tiling's refresh names its sources itself -- a concat every cell -- so they are among the handles that step reads;
    # the solves count as writers of their tiling: the kept schedule a later solve uses was built by one of them)

    def with_operands(hs):   # (a plan reads its operands' values whenever it runs, not only when it is made; so does a solver --
        out = set(hs)        # its A, its factor, its hierarchy and that one's A -- and a hierarchy)
        while True:
            more = out | {t for h in out for t in operands.get(h, ())}
            if more == out:
                return out
            out = more

    want = with_operands(live if live is not None else handles(prog[step])[0])
    keep = [] if live is not None else [step]
    for i in range(step - (0 if live is not None else 1), -1, -1):
        read, wrote = handles(prog[i])
        if wrote & want:
            keep.append(i)
            want |= with_operands(read)
    return sorted(keep)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seed", type=int)
    ap.add_argument("--steps", type=int)
    ap.add_argument("--program")
    ap.add_argument("--context", choices=("session", "torch_stream", "graph_replay"))
    args = ap.parse_args()
    if (args.seed is None) == (args.program is None):
        ap.error("give --seed or --program")
    import torch

    import __graft_entry__ as g
    import seqgen as sg
    import seqrun
    pkg = g.load_package()
    if args.program:
        prog = sg.loads(open(args.program).read())
    else:
        prog = sg.program(args.seed, args.steps or sg.STEPS)
    kind = args.context or (sg.context_kind(args.seed) if args.seed is not None else "session")
    print(f"{len(prog)} steps on a {kind} context")
    if kind == "torch_stream":
        stream = torch.cuda.Stream()
        torch.cuda.set_stream(stream)
        ctx = pkg.Context(0, stream=stream.cuda_stream)
    else:
        ctx = pkg.Context(0)
        ctx.set_graph_replay(kind == "graph_replay")
    status = 0
    with tempfile.TemporaryDirectory() as tmp:
        runner = seqrun.Runner(pkg, ctx, tmp, on_stream=kind == "torch_stream", log=print)
        try:
            runner.run(prog, args.seed)
            print(f"all {len(prog)} steps and {runner.audits} audits match the model")
        except seqrun.SeqGpuError as e:
            print(f"GPU error, nothing more is run:\n{e}")
            status = 2
        except seqrun.SeqMismatch as e:
            print(e)
            live = None if e.where == "step" else [h for h in list(runner.m.t) + list(runner.m.p) + list(runner.m.k) + list(runner.m.h)]
            if e.where == "after the refusal":
                live = [h for h in e.rec[1] if h is not None]
            keep = closure(prog, e.step, live)
            print(f"\ndependency closure of step {e.step} ({len(keep)} of {e.step + 1} steps):")
            print(sg.dumps([prog[i] for i in keep]))
            status = 1
    ctx.close()
    return status


if __name__ == "__main__":
    sys.exit(main())
