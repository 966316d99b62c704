"""GPU: random operation sequences on one context against a host model ("Sequence test").

Every other GPU test file takes fresh handles through one feature in a fixed order.  This one runs the library's operations in
orders nobody wrote down, on handles that already have a history, on a context whose scratch something else has used: for each
committed seed, tests/seqgen.py writes a program (a list of operations on a pool of at most 8 tilings and 4 plans), and
tests/seqrun.py executes it step by step on the device and on the host model of tests/seqmodel.py, comparing after every step and
auditing every live handle every 10 steps.  Every comparison is bit for bit over every entry (NaN == NaN; +0 == -0 under min / max
only); the model computes nothing itself: every value comes from the references of the feature tests (the oracle, semiringref,
maskref, ewiseref, selectref, mxvref, spmmref, sddmmref).

Three seed lists: seqgen.SEEDS draws from the operation set the test was added with (its programs are pinned by digest in
tests/test_seq_cpu.py), seqgen.SEEDS2 from the second set, which adds apply, scale, transpose, extract, assign, kron, concat, build
and ilu0 with their refreshes, select_topk, sampled_mxm and its in-place writer, the frontier and arg folds, bfs, bfs_parents,
triangle_count, trsv, lu_solve, trsv_info and ilu0_info (references: applyref, extractref, assignref, kronref, concatref, buildref,
topkref, sampledref, frontierref, argref, trsvref, ilu0ref).  The audit also
compares trsv_info of every triangle whose schedule the model has as built, and a factor's ilu0_info.

seqgen.SEEDS3 draws from the third set: everything the second has, plus the graph routines (colour, colour_order on a colouring and
on component ids, components, mis, aggregate; seeds 0 and 12345, the "equal" and "ties" priority arrays from the host and from the
device), solvers (krylov_create / _solve / _close and Tiled.solve: CG and BiCGStab with no, the diagonal, an LU and the multigrid
preconditioner) and hierarchies (amg_create over tests/amgcases.py's option grid, refresh, apply, info, a borrowed A_l / P_l / R_l
handed to mxv, reduce, export_csr or a graph routine), in two new pools of at most 3 solvers and 2 hierarchies (references:
colourref, ccref, aggref, krylovref, amgref).  Every output buffer holds a poison value before the call; every element, every count,
every field of a solve's result (launches from the header's formula, with the trsv launches the device reports) and the written
part of the history are compared bit for bit, the rest of the history must still be poison.  The audit compares every live
hierarchy's info fields (bytes: not negative, nothing more) and every level's A_l, P_l, R_l with the model, in which a refresh is a
rebuild from the current values.  A graph call whose scratch demand does not exceed the largest any graph call has made on the
context must allocate nothing (seqrun.Runner._graph_call; Context.trim does not release that scratch).  Three scenarios are
scripted into the random order: the life of a solver, the life of a hierarchy, the colour reordering.

Each seed list runs on three kinds of context, eight seeds each: the session context, one on a non-default torch stream (torch
tensors and library calls with no synchronisation between them), and one with graph replay on.

PEM_SEQ_SEED (and PEM_SEQ_STEPS, default seqgen.STEPS) in the environment make this file run that one program instead of the
committed lists (a seed from seqgen.SET2_FROM on draws from the second set, one from seqgen.SET3_FROM on from the third);
tools/seq_replay.py replays a program from the text a failure prints.

Negative controls: nine deliberate mistakes of the MODEL (seqmodel.MUTATIONS; the library is never touched, nothing can fault)
must each make the runner report a mismatch, at the step tests/seqcontrol.py computes from the models alone.

Left out, and why: the multi-GPU entry points (pem_mgpu_*, their own contexts and ranks: test_gpu_multirank.py); matgen's
million-row cases (k64_bins, wide_tilecols, xl_mixed_AAt, hub_tile_2100_AAt, blockrows_10000: the numpy references take seconds
per call there); duplicate runs longer than BUILD_INORDER_MAX under plus / times and set_values_sampled_mxm with accumulate under
plus_pair (the header lets both round differently from the references); refusals of trsv_info / ilu0_info; false symmetric = 1
promises (the header leaves their outcome open: the feature tests pin what it does say); pem_amg_info's bytes (it depends on the
context's history); the launches of a Tiled.solve that makes its own factor (its trsv launches are not to be had); the CLI and its
stages; the export_*_device forms, flop_count and the tile-row split helpers (read-only, no kept state);
pem_cplan_info's ntiles_c / npairs (they depend on the options; prune_ref checks them in test_gpu_sweep.py); PEM_OPT_S1_XLCAP,
S1_SERIAL, STEP1_GLOBAL_SORT, WARM, EXPORT_ROWS and S3_POISON of the options; writers on a tiling without entries and the
destruction of a tiling another live handle names (the header leaves both outcomes open); kernel profiling.

Wall time, measured on one MI355X in one session: this file (72 programs x 120 steps and the nine negative controls) 24.7 s,
tests/test_gpu_sddmm.py (the yardstick the lists are sized against) 16.7 s, no program above 0.6 s; with the first two lists it was
15.8 s against 16.8 s, with the first list alone 8.1 s against 17.5 s.  A single seed in a process of its own takes about 3 s, most
of it start-up.  The CPU-only model runs of the first two lists take about 10 s together in tests/test_seq_cpu.py (the model alone:
2.2 s); the third list's take about 9 s there (the model alone: 2.0 s).
"""
import os

import pytest
import torch

import seqcontrol
import seqgen as sg
import seqrun

pytestmark = pytest.mark.gpu

torch.cuda.is_available()   # (torch's runtime first, as in the other GPU files)

if os.environ.get("PEM_SEQ_SEED"):
    SEEDS = (int(os.environ["PEM_SEQ_SEED"]),)
    STEPS = int(os.environ.get("PEM_SEQ_STEPS") or sg.STEPS)
else:
    SEEDS, STEPS = sg.SEEDS + sg.SEEDS2 + sg.SEEDS3, sg.STEPS


class _Contexts:
    """the three context kinds, made on first use and kept for the module (so that a program meets a used context)"""

    def __init__(self, pkg, session_ctx):
        self.pkg, self.made, self.prev = pkg, {"session": session_ctx}, None

    def get(self, kind):
        if kind not in self.made:
            if kind == "torch_stream":
                self.prev = torch.cuda.current_stream()
                self.stream = torch.cuda.Stream()
                self.made[kind] = self.pkg.Context(0, stream=self.stream.cuda_stream)
            else:
                self.made[kind] = self.pkg.Context(0)
                self.made[kind].set_graph_replay(True)
        return self.made[kind]

    def run(self, kind, seed, steps, tmpdir, mutations=()):
        ctx = self.get(kind)
        on_stream = kind == "torch_stream"
        if on_stream:
            torch.cuda.set_stream(self.stream)
        try:
            return seqrun.Runner(self.pkg, ctx, tmpdir, on_stream=on_stream, mutations=mutations).run(sg.program(seed, steps), seed)
        finally:
            if on_stream:
                torch.cuda.set_stream(self.prev)

    def close(self):
        for kind, c in self.made.items():
            if kind != "session":
                c.close()


@pytest.fixture(scope="module")
def contexts(pkg, ctx):
    c = _Contexts(pkg, ctx)
    yield c
    c.close()


@pytest.mark.parametrize("seed", SEEDS, ids=[f"seed{s}_{sg.context_kind(s)}" for s in SEEDS])
def test_program_matches_the_model(contexts, tmp_path, seed):
    assert contexts.run(sg.context_kind(seed), seed, STEPS, tmp_path) == STEPS


@pytest.mark.parametrize("mutation", sorted(seqcontrol.NEGATIVE))
def test_negative_control_is_detected(contexts, tmp_path, mutation):
    """a deliberate mistake of the model (never of the library) makes the runner report a mismatch, at the expected step"""
    seed, (step, where) = seqcontrol.NEGATIVE[mutation]
    with pytest.raises(seqrun.SeqMismatch) as e:
        contexts.run(sg.context_kind(seed), seed, sg.STEPS, tmp_path, mutations=(mutation,))
    assert (e.value.step, e.value.where) == (step, where), str(e.value)
    assert f"seed {seed}" in str(e.value) and sg.loads(str(e.value)) == sg.program(seed, step + 1)
