"""Seeded generator of operation programs for the sequence test (tests/seqmodel.py is the host model, tests/seqrun.py the runner).

program(seed, steps) is a pure function of its arguments: a list of records (op, handle ids, arguments) drawn with
numpy.random.default_rng(seed).  While it draws, the generator runs the host model on the program so far: that is its shadow of
the pool, so every emitted record is well-typed (shapes and value types agree, the handles are alive) and its outcome is one the
header documents.  A record whose arguments carry "expect" is a deliberate refusal (the value names which rule refuses it); every
other record is accepted by the model.  Nothing is emitted whose outcome include/pem_spgemm.h leaves open: no destroy of a tiling a
live plan or a live derived tiling names, no writer on a tiling without entries (whether that bumps the value version is not
stated), no call that is wrong in two ways at once.

Handles get old: the pool holds at most 8 tilings and 4 plans, operations on existing handles outnumber creations, the tiling
written last is read next more often than not, and kinds the program has used least are preferred (so a short seed list reaches
every kind in both value types).

Text form: one JSON array [op, [ids], {arguments}] per line (dumps / loads); tools/seq_replay.py reads it back.

Three operation sets.  A seed below SET2_FROM draws from the first set (_Gen), and program() returns for it what it returned when
the sequence test was added (tests/golden/seq_program_digests.json holds the digests of SEEDS' programs).  A seed from SET2_FROM
on draws from the second set (_Gen2; SEEDS2 is its committed list): everything the first has, plus
  derivations with a refresh   apply, scale, transpose, extract, assign, kron, concat, build / build_device (keep_map), ilu0,
                               each with its set_values_from_*
  derivations without one      select_topk, sampled_mxm, a build without a map; split, emitted as its extracts (d_extract draws
                               pieces of a partition by ranges, which is what Tiled.split emits)
  a writer                     set_values_sampled_mxm (every semiring, transpose_b, with and without accumulate)
  dense readers                triangle_count (on symmetric patterns),               mxv_frontier, mxv_arg, reduce_arg, bfs, bfs_parents, trsv, lu_solve, trsv_info, ilu0_info
and the refusals of REFUSALS2.  Boundary values (powi's 1, 2, 64; top-k's k = 0, 1, the line length and beyond; the dup ops;
run lengths either side of BUILD_INORDER_MAX; the concat shapes) come from the feature tests' lists.  Square matrices that store their
diagonal come from tests/trsvcases.py, tests/ilu0cases.py (hubs_1600 rarely) and random ones with the diagonal forced in.  Three
scenarios are scripted into the random order and interleaved with it (start_scenario2): a chain of three derivations refreshed
link by link, the life of a factor, a concat between refreshes.

Special values in the second set: trsv, lu_solve and ilu0 run on whatever values the program wrote last, the inf / NaN / zero /
subnormal mix included -- trsvref and ilu0ref are bit-exact there (NaN equals NaN; test_gpu_trsv.py and test_gpu_ilu0.py check
zero pivots, infinities and NaN by bits), so no special value is left out of them.

Left out, because the header lets the library round differently from the references there: runs of duplicates longer than
BUILD_INORDER_MAX under plus and times (they may be regrouped; the other six dup ops get such runs), and set_values_sampled_mxm
with accumulate under plus_pair (a tile pair's count enters in one addition).  Also left out: refusals of trsv_info / ilu0_info.

A seed from SET3_FROM on draws from the third set (_Gen3; SEEDS3 is its committed list): everything the second has, plus
  graph readers                colour (seeds 0 and 12345, the "equal" and "ties" priority arrays of test_gpu_colour.py, each from the
                               host and from the device), colour_order (on a colouring, and on component ids with ncolours =
                               ncomponents), components (with and without ids), mis (distances 1 and 2), aggregate (with and
                               without roots)
  solvers                      krylov_create (CG or BiCGStab; none, diag, lu, or amg through pem_krylov_create_amg; check_every is
                               an option of create: 1, 3, 8 or above max_iters), krylov_solve (with and without history and guess),
                               krylov_close, tiled_solve (the Tiled.solve convenience)
  hierarchies                  amg_create (tests/amgcases.py's option grid, refreshable 0 / 1), amg_refresh, amg_apply, amg_info,
                               amg_level (a borrowed A_l, P_l or R_l handed to mxv, reduce, export_csr or a graph routine), amg_close
in two pools of their own (MAX_SOLVERS, MAX_HIERARCHIES), and the refusals of REFUSALS3.  The rules the third set keeps: symmetric =
1 only where the model knows the pattern to be symmetric; no tiling destroyed that a live solver or hierarchy names, no hierarchy
that a live solver names; a borrowed level handle is read within its record only.  Solves run on whatever values the program wrote
last (krylovref follows the header's NONFINITE and BREAKDOWN line by line); max_iters is at most 30.  Graphs and systems: the
matgen cases, colourref.built_graphs(), tests/amgcases.py's systems (krylovcases' among them), the smallest weighted most.  Three
scenarios (start_scenario3): the life of a solver (ilu0, krylov_create lu, solve, a writer on A, set_values_from_ilu0, solve, a graph
routine on another tiling, solve), the life of a hierarchy (amg_create, krylov_create amg, solve, a writer on A, amg_refresh, solve,
trim or reserve, amg_apply, amg_refresh, amg_info), the reorder (colour, colour_order, extract with the permutation as both lists,
ilu0, trsv_info, a solver on the reordered matrix and its solve).  r_provenance is an owed draw as r_needy's: the third set's kinds
leave the second's derivations fewer draws, so a program makes the derived tilings its graph routines have not met yet.

The second set's pool holds MAX_TILINGS2 = 10 tilings (more kinds of derived tilings have to be alive at once).  Most of its draws
go to r_needy, which serves the (kind, value type) a program ran least in a fixed round that every program enters at its own
place: that, not chance, is what lets 24 x 120 steps reach every new kind ten times in both value types.  The first set's kinds
keep a share (conversions, writers, plans and readers through the categories, ewise / select / sddmm / from_cplan / save_load
through a draw of their own), so the new readers and refreshes also meet sources that an old feature wrote last; the step-wise
plan calls, set_semiring and the exports are drawn rarely here -- the first set covers them.
"""
import json

import numpy as np

import applyref
import argref
import buildref
import ewiseref
import kronref
import selectref
import seqmodel as sm
import topkref
from semiringref import SEMIRINGS

MAX_TILINGS, MAX_PLANS = 8, 4
CASES = ("tiny_9x9", "rand_50", "rand_300", "rect_70x40_AAt", "rect_33x65_AAt", "ragged_37", "dense_tile", "dense_48", "empty_rows",
         "empty_matrix", "powerlaw_600", "band_1500", "blockrows_1600", "hub_row_4000")
CASE_WEIGHT = (3, 3, 3, 3, 3, 3, 2, 2, 2, 1, 1.5, 1, 0.7, 0.7)
DIMS = (1, 9, 16, 33, 40, 48, 65, 70, 129, 300)                       # shapes of the random matrices (with the cases' own)
DENSITIES = (0.002, 0.01, 0.05, 0.3)                                  # test_gpu_sweep.py's
SPMM_KS = (1, 3, 4, 5, 7, 8, 9, 13, 15, 16, 17, 21, 37, 69)           # test_gpu_spmm.py's boundary list
SDDMM_KS = (0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 32, 33, 40)           # test_gpu_sddmm.py's
OPTION_VALUES = dict(prune=(0, 1), wide=(0, 1), s3_band=(0, 1), s3_decode=(0, 1), s3_epw=(0, 1, 2, 4), s3_idx64=(0, 1), s3_mark=(0, 1),
                     s3_xcd=(0, 1), s2_transposed=(0, 1, 2), s1_segments=(0, 1), s1_xl_global=(0, 1), s1_force_key64=(0, 1))
SCALES = (1.0, -1.0, 2.0, 0.5)
VALUE_THUNKS = (0.0, 0.25, -0.5, 1.0, -1.0, 0.5)
RESERVES = (1 << 20, 1 << 24, 1 << 26)
# size guards of the numpy references: scalar products of a plan, entries of a tiling made from a C, dense elements of one call
MAX_PRODUCTS, MAX_C_NNZ, MAX_DENSE_WORK = 400_000, 150_000, 1_500_000
REFUSALS = ("export_not_current", "from_cplan_not_current", "refresh_plan_not_current", "wrong_plan", "wrong_ewise_source",
            "wrong_select_source", "select_by_value_refresh", "step_out_of_order", "masked_plan_option")
CONTEXT_KINDS = ("session", "torch_stream", "graph_replay")
# the committed programs: seed i of the list runs on context kind CONTEXT_KINDS[i % 3] (8 seeds per kind)
SEEDS = tuple(range(101, 125))
STEPS = 120

# ---- the second operation set (_Gen2): seeds from SET2_FROM on draw from it; SEEDS2 is dealt to the context kinds as SEEDS is
SET2_FROM = 1000
# How SEEDS2 was found: with the weights below, runs of 24 consecutive seeds starting at 1201, 1301, ... were tried against
# test_second_set_coverage_conditions (tests/test_seq_cpu.py); about half of them meet every condition (1201, 1301, 1401, 1701,
# 1901 of the first ten), and 1401 was taken.  After a change to the weights, BOOST2 or a draw: search
# again the same way, then take the three figures of seqcontrol.NEGATIVE from seqcontrol.first_divergence.
SEEDS2 = tuple(range(1401, 1425))
TRSV_CASES = ("dense_1", "dense_15", "dense_16", "dense_17", "dense_33", "bidiagonal_200", "arrow_400", "wide_thin_wide",
              "grid_40x40_red_black", "random_600")                  # tests/trsvcases.py's
TRSV_WEIGHT = (1, 2, 2, 3, 3, 2, 1.5, 0.7, 0.7, 1)
ILU0_CASES = ("dense_1", "dense_15", "dense_16", "dense_17", "dense_33", "tridiagonal_200", "band_100_20", "grid_40x40_red_black",
              "wide_thin_wide", "double_arrow_400", "random_300", "hubs_1600")   # tests/ilu0cases.py's
ILU0_WEIGHT = (1, 2, 2, 3, 3, 2, 1.5, 0.7, 0.7, 1, 1.5, 0.15)
CONCAT_SHAPES = ("1xn", "nx1", "2x2", "none_cell", "same_twice", "zero_strip")
# size guards of the second set: entries of a solve or a factor (trsvref and ilu0ref walk them in Python), ilu0ref's inner steps,
# nnz(A) * nnz(B) of a kron, the entries of a concat, the larger dimension of either, the length of an index list in a record
MAX_TRSV_NNZ, MAX_ILU0_COST, MAX_KRON_NNZ, MAX_CONCAT_NNZ, MAX_DIM2, MAX_LIST = 30_000, 200_000, 40_000, 60_000, 6000, 300
KINDS2_T = ("build", "build_device", "set_values_from_build", "sampled_mxm", "set_values_sampled_mxm", "triangle_count", "apply", "set_values_from_apply", "scale", "set_values_from_scale", "assign", "set_values_from_assign", "select_topk",
            "mxv_frontier", "mxv_arg", "reduce_arg", "bfs", "bfs_parents", "transpose", "set_values_from_transpose", "extract", "set_values_from_extract", "kron",
            "set_values_from_kron", "concat", "set_values_from_concat", "ilu0", "set_values_from_ilu0", "trsv", "lu_solve", "trsv_info",
            "ilu0_info")
REFUSALS2 = ("wrong_kind_refresh", "wrong_source_refresh", "concat_swapped", "concat_wrong_count", "trsv_nonsquare", "ilu0_nonsquare",
             "trsv_missing_diag", "ilu0_missing_diag", "trsv_overlap", "powi_thunk", "extract_empty_device", "assign_repeat_device", "build_refresh_no_map",
             "build_refresh_wrong_nnz")
MAX_TILINGS2 = 10                      # the second set's pool: more kinds of derived tilings have to be alive at once
MAX_SAMPLED_WORK = 300_000             # matched-pair candidates of one sampled product (sampledref lists them all)
BOOST2 = dict(build_refresh_no_map=8.0, build_refresh_wrong_nnz=3.0, concat_swapped=3.0, ilu0_info=14.0, lu_solve=9.0, kron=4.0, ilu0=6.0, assign=3.0, concat=1.5, trsv_info=30.0, bfs=14.0, bfs_parents=12.0, apply=1.5, transpose=1.5, extract=2.0, select_topk=1.5,
              set_values_from_extract=2.0)

# ---- the third operation set (_Gen3): seeds from SET3_FROM on draw from it; SEEDS3 is dealt to the context kinds as SEEDS is
SET3_FROM = 2000
# How SEEDS3 was found: as SEEDS2 was -- with the weights below, runs of 24 consecutive seeds starting at 2001, 2101, ... were tried
# against test_third_set_coverage_conditions (tests/test_seq_cpu.py); three of the first five meet every condition (2101, 2201, 2301;
# 2001 has no graph routine on a tiling made from a plan, 2401 no mis on a non-square tiling), and 2101 was taken.  After a change to
# the weights or a draw: search again the same way, then take the figures of the third set's controls in seqcontrol.NEGATIVE from
# seqcontrol.first_divergence.
SEEDS3 = tuple(range(2101, 2125))
MAX_SOLVERS, MAX_HIERARCHIES = 3, 2     # the third set's two pools
GRAPH_SOURCES = ("k70_in_75", "k131", "path_203_one_way")            # colourref.built_graphs(): window overflow, column direction
SYSTEMS = ("spd_dense_1", "spd_dense_15", "spd_dense_17", "spd_dense_33", "diag_50", "spd_tridiagonal_200", "gen_tridiagonal_200", "gen_dense_33",
           "poisson_40", "spd_tridiagonal_4097")                     # tests/amgcases.py's (krylovcases' among them), the smallest weighted most
SYSTEM_WEIGHT = (1, 1.5, 3, 3, 3, 3, 2, 2, 1.5, 0.05)
MAX_ITERS3 = (0, 1, 2, 3, 5, 8, 13, 30)
RTOLS, ATOLS = (1e-8, 1e-4, 1e-2), (0.0, 0.0, 1e-3)
AMG_SMOOTH, AMG_COARSE, AMG_SWEEPS = (0, 1), (8, 40), ((1, 4), (2, 1))   # tests/amgcases.py's option grid
# size guards of the third set: entries of a graph (colourref and aggref walk them in Python), entries of a solve's A times max_iters
# (of its factor: trsvref walks them in Python), the entries and the scalar products (sum of squared row lengths) of a hierarchy's A
MAX_GRAPH_NNZ, MAX_SOLVE_WORK, MAX_LU_WORK, MAX_AMG_NNZ, MAX_AMG_PRODUCTS = 30_000, 250_000, 60_000, 13_000, 120_000
GRAPH_KINDS = sm.GRAPH_KINDS
SOLVER_KINDS = ("krylov_create", "krylov_solve", "krylov_close", "tiled_solve")
AMG_KINDS = ("amg_create", "amg_refresh", "amg_apply", "amg_info", "amg_level", "amg_close")
KINDS3_T = GRAPH_KINDS + SOLVER_KINDS + AMG_KINDS
NEEDY3_SHARE = dict(krylov_solve=3.0, amg_apply=1.5, amg_refresh=2.0, amg_level=1.5, krylov_close=0.7, amg_close=0.6)
PRIORITIES = ("seed_0", "seed_12345", "equal_host", "equal_device", "ties_host", "ties_device")
METHOD_PRECOND = tuple((m, p) for m in ("cg", "bicgstab") for p in ("none", "diag", "lu", "amg"))
REFUSALS3 = ("colour_nonsquare", "components_nonsquare", "mis_nonsquare", "aggregate_nonsquare", "krylov_nonsquare", "mis_distance_3",
             "lu_no_factor", "factor_other_precond", "factor_other_dtype", "amg_other_matrix", "amg_missing_diag", "refresh_not_refreshable",
             "solve_wrong_form", "priority_overlap")

KINDS_T = ("from_coo", "from_csr", "from_coo_device", "set_values", "set_values_device", "set_values_from_cplan", "set_values_from_ewise",
           "set_values_from_select", "set_values_sddmm", "from_cplan", "ewise", "select", "sddmm", "mxv", "reduce", "spmm", "save_load", "close")
KINDS_P = ("plan_create", "step1", "step2", "step3", "spgemm", "set_semiring", "set_option", "export_csr", "export_coo", "plan_close")
KINDS_CTX = ("trim", "reserve", "synchronize")
# kinds that are possible on few pools only are taken more often where they are possible
BOOST = dict(set_values_from_cplan=6.0, set_values_from_select=6.0, from_cplan=4.0, export_csr=7.0, export_coo=9.0,
             step2=3.0, ewise=2.0, select=2.0, set_values_from_ewise=0.5, sddmm=1.5, save_load=1.5, refresh_plan_not_current=8.0, select_by_value_refresh=5.0, wrong_plan=2.0)


def dumps(prog):
    return "\n".join(json.dumps([op, list(ids), args], sort_keys=True) for op, ids, args in prog)


def loads(text):
    out = []
    for line in text.splitlines():
        line = line.strip()
        if line.startswith("["):
            op, ids, args = json.loads(line)
            out.append((op, tuple(ids), args))
    return out


def record_dtype(model, rec):
    """the value type a record works in ("f64" / "f32"; None for the context's own calls), read off the model BEFORE the record runs"""
    op, ids, a = rec
    if op in KINDS_CTX:
        return None
    if "dtype" in a:
        return a["dtype"]
    h = ids[0]
    if h in model.k or h in model.h:     # a solver or a hierarchy: the value type of its A
        h = (model.k[h] if h in model.k else model.h[h]).a
    return sm.dtname(model.p[h].A.dtype if h in model.p else model.t[h].dtype)


class _Gen:
    MAX_T = MAX_TILINGS               # the pool's tilings (the second set takes more)

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.m = sm.Model()
        self.prog = []
        self.nt = self.np_ = 0
        self.count = {}
        self.refusals = 0
        self.hot = None                  # the tiling written last
        self.script = []                 # pending records of the plan scenario (see _scenario)
        self.scenarios = 0

    # ---- draws -------------------------------------------------------------------------------------------------------------
    def pick(self, seq, weights=None):
        seq = list(seq)
        if weights is None:
            return seq[int(self.rng.integers(len(seq)))]
        w = np.asarray(weights, float)
        return seq[int(self.rng.choice(len(seq), p=w / w.sum()))]

    def chance(self, p):
        return bool(self.rng.random() < p)

    def seed(self):
        return int(self.rng.integers(1 << 30))

    def vals_args(self):
        return dict(seed=self.seed(), special=self.chance(0.25))

    def least(self, kinds, dtype):
        """one of `kinds`, those the program used least in this value type first"""
        w = [BOOST.get(k, 1.0) / (1 + self.count.get((k, dtype), 0)) ** 2 for k in kinds]
        return self.pick(kinds, w)

    # ---- the pool ----------------------------------------------------------------------------------------------------------
    def tilings(self, pred=lambda T: True):
        return [i for i, T in self.m.t.items() if pred(T)]

    def plans(self, pred=lambda p: True):
        return [i for i, p in self.m.p.items() if pred(p)]

    def named(self, tid):
        """a live plan or a live derived tiling names this tiling"""
        T = self.m.t[tid]
        if any(T is p.A or T is p.B or T is p.M for p in self.m.p.values()):
            return True
        return any(D.prov is not None and D.prov[0] in ("ewise", "select") and tid in D.prov[1:3] for D in self.m.t.values())

    def new_t(self):
        self.nt += 1
        return f"t{self.nt}"

    def new_p(self):
        self.np_ += 1
        return f"p{self.np_}"

    def want_dtype(self):
        n64 = sum(v for (k, d), v in self.count.items() if d == "f64")
        n32 = sum(v for (k, d), v in self.count.items() if d == "f32")
        return "f64" if n64 <= n32 else "f32"

    # ---- records: each returns a record or None when the pool offers no operand ----------------------------------------------------
    def r_convert(self, dtype):
        if len(self.m.t) >= self.MAX_T:
            return self.r_close(dtype)
        op = self.least(("from_coo", "from_csr", "from_coo_device"), dtype)
        peers = self.tilings(lambda T: sm.dtname(T.dtype) == dtype and T.rows * T.cols > 0)
        if peers and self.chance(0.75):
            T = self.m.t[self.pick(peers)]
            how = self.pick(("same", "right", "left"))
            rows, cols = {"same": (T.rows, T.cols), "right": (T.cols, self.pick(DIMS + (T.rows,))), "left": (self.pick(DIMS + (T.cols,)), T.rows)}[how]
        else:
            if self.chance(0.7):
                src = {"case": self.pick(CASES, CASE_WEIGHT)}
                return (op, (), dict(out=self.new_t(), src=src, dtype=dtype, transpose=op != "from_csr" and self.chance(0.4)))
            rows, cols = self.pick(DIMS), self.pick(DIMS)
        if rows * cols > 200_000:        # (the cases' own large shapes: a sparse random matrix of that shape)
            nnz = int(self.pick((2, 6, 12)) * max(rows, cols))
        else:
            nnz = max(1, int(rows * cols * self.pick(DENSITIES)))
        transpose = op != "from_csr" and self.chance(0.4)
        if transpose:
            rows, cols = cols, rows      # (the tiling is of the transposed source)
        src = {"rand": [self.seed(), int(rows), int(cols), int(nnz), bool(self.chance(0.35))]}
        return (op, (), dict(out=self.new_t(), src=src, dtype=dtype, transpose=transpose))

    def r_close(self, dtype):
        free = [i for i in self.tilings(lambda T: sm.dtname(T.dtype) == dtype) if not self.named(i)] or [i for i in self.tilings() if not self.named(i)]
        if not free:
            return self.r_plan_close(dtype)
        # a derived tiling that was never refreshed goes last
        w = [0.1 if self.m.t[i].prov is not None and self.m.t[i].version == 0 and self.m.t[i].nnz else 1.0 for i in free]
        return ("close", (self.pick(free, w),), {})

    def r_chase(self, dtype):
        """the refresh of a derived tiling, the (kind, value type) the program ran least first: these are possible on few pools only"""
        cand = []
        for i, T in self.m.t.items():
            if T.prov is None or T.nnz == 0:
                continue
            kind = "set_values_from_" + T.prov[0]
            ok = (T.prov[1] in self.m.p) if T.prov[0] == "cplan" else (T.prov[1] in self.m.t and (T.prov[2] in self.m.t if T.prov[0] == "ewise"
                                                                                               else T.prov[2] in selectref.POSITIONAL))
            if ok:
                cand.append((self.count.get((kind, sm.dtname(T.dtype)), 0), i))
        if not cand:
            return None
        low = min(c for c, _ in cand)
        return self.r_writer(None, self.pick([i for c, i in cand if c == low]), refresh=True)

    def r_plan_close(self, dtype):
        ps = self.plans()
        made = {T.prov[1] for T in self.m.t.values() if T.prov is not None and T.prov[0] == "cplan"}
        ps = [i for i in ps if i not in made] or ps          # (a plan a live tiling was made from goes last: its refresh needs it)
        return ("plan_close", (self.pick(ps),), {}) if ps else None

    def r_plan_create(self, dtype, operand=None):
        if len(self.m.p) >= MAX_PLANS:
            return self.r_plan_close(dtype)
        pairs = []
        for ia, A in self.m.t.items():
            for ib, B in self.m.t.items():
                if A.dtype == B.dtype and sm.dtname(A.dtype) == dtype and A.cols == B.rows and (operand is None or operand in (ia, ib)) \
                        and self.m.products(A, B) <= MAX_PRODUCTS:
                    pairs.append((ia, ib))
        if not pairs:
            return None
        ia, ib = self.pick(pairs)
        A, B = self.m.t[ia], self.m.t[ib]
        masks = self.tilings(lambda M: (M.rows, M.cols) == (A.rows, B.cols))
        im = self.pick(masks) if masks and self.chance(0.45) else None
        lo, hi = 0, -1
        if A.tile_rows >= 2 and self.chance(0.25):
            lo = int(self.rng.integers(0, A.tile_rows - 1))
            hi = int(self.rng.integers(lo + 1, A.tile_rows + 1))
        semiring = self.pick(SEMIRINGS) if self.chance(0.5) else "plus_times"
        return ("plan_create", (ia, ib, im), dict(out=self.new_p(), complement=im is not None and self.chance(0.4), lo=lo, hi=hi, semiring=semiring))

    def r_plan_op(self, dtype, pid=None):
        ps = [pid] if pid is not None else self.plans(lambda p: sm.dtname(p.A.dtype) == dtype)
        if not ps:
            return self.r_plan_create(dtype)
        pid = self.pick(ps)
        p = self.m.p[pid]
        kinds = ["spgemm", "step1", "set_semiring", "set_option"]
        if p.state >= 1:
            kinds.append("step2")
        if p.state >= 2:
            kinds.append("step3")
        if self.m.current(p):
            kinds += ["export_csr", "export_coo"]
            if len(p.C[1]) <= MAX_C_NNZ and len(self.m.t) < self.MAX_T:
                kinds += ["from_cplan"]
        op = self.least(kinds, dtype)
        if op == "set_semiring":
            return (op, (pid,), dict(semiring=self.pick(SEMIRINGS)))
        if op == "set_option":
            return self.r_set_option(pid)
        if op == "from_cplan":
            return (op, (pid,), dict(out=self.new_t(), transpose=self.chance(0.5)))
        return (op, (pid,), {})

    def r_export(self, dtype):
        ps = self.plans(lambda p: sm.dtname(p.A.dtype) == dtype)
        if not ps:
            return self.r_plan_create(dtype)
        cur = [i for i in ps if self.m.current(self.m.p[i])]
        if not cur:
            return ("spgemm", (self.pick(ps),), {})
        return (self.least(("export_csr", "export_coo"), dtype), (self.pick(cur),), {})

    def r_set_option(self, pid):
        p = self.m.p[pid]
        name = self.pick(sorted(OPTION_VALUES))
        vals = [v for v in OPTION_VALUES[name] if not (p.M is not None and name == "wide" and v == 0)]
        other = [v for v in vals if v != p.options[name]]
        value = self.pick(other) if other and self.chance(0.9) else self.pick(vals)
        return ("set_option", (pid,), dict(name=name, value=int(value)))

    def r_writer(self, dtype, tid=None, refresh=False):
        ts = [tid] if tid is not None else self.tilings(lambda T: sm.dtname(T.dtype) == dtype and T.nnz > 0)
        ts = [i for i in ts if self.m.t[i].nnz > 0]
        if not ts:
            return None
        # prefer tilings a refresh is possible for
        cand = []
        for i in ts:
            T = self.m.t[i]
            cand += [("set_values", i), ("set_values_device", i)]
            if T.nnz * 17 <= MAX_DENSE_WORK:
                cand.append(("set_values_sddmm", i))
            if T.prov is not None:
                if T.prov[0] == "cplan" and T.prov[1] in self.m.p:
                    cand.append(("set_values_from_cplan", i))
                if T.prov[0] == "ewise" and T.prov[1] in self.m.t and T.prov[2] in self.m.t:
                    cand.append(("set_values_from_ewise", i))
                if T.prov[0] == "select" and T.prov[1] in self.m.t and T.prov[2] in selectref.POSITIONAL:
                    cand.append(("set_values_from_select", i))
        kinds = sorted({k for k, _ in cand if not refresh or "_from_" in k})
        op = self.least(kinds, dtype if tid is None else sm.dtname(self.m.t[tid].dtype))
        i = self.pick([t for k, t in cand if k == op])
        T = self.m.t[i]
        if op in ("set_values", "set_values_device"):
            # the order the program wrote least on any tiling comes first
            order = self.least(("row", "col"), "order")
            self.count[(order, "order")] = self.count.get((order, "order"), 0) + 1
            return (op, (i,), dict(order=order, **self.vals_args()))
        if op == "set_values_sddmm":
            return (op, (i,), dict(semiring=self.pick(SEMIRINGS), k=self.sddmm_k(T), accumulate=self.chance(0.5), **self.vals_args()))
        if op == "set_values_from_cplan":
            if not self.m.current(self.m.p[T.prov[1]]):      # (first make the plan's C current again; the refresh comes on a later draw)
                return ("spgemm", (T.prov[1],), {})
            return (op, (i, T.prov[1]), {})
        if op == "set_values_from_ewise":
            return (op, (i, T.prov[1], T.prov[2]), {})
        return (op, (i, T.prov[1]), {})

    def sddmm_k(self, T):
        return int(self.pick([k for k in SDDMM_KS if max(T.nnz, T.rows, T.cols) * (k + 11) <= MAX_DENSE_WORK] or [0]))

    def r_derive(self, dtype):
        if len(self.m.t) >= self.MAX_T:
            return self.r_close(dtype)
        op = self.least(("ewise", "select", "sddmm", "from_cplan", "save_load"), dtype)
        ts = self.tilings(lambda T: sm.dtname(T.dtype) == dtype)
        if op == "from_cplan":
            ps = self.plans(lambda p: sm.dtname(p.A.dtype) == dtype and self.m.current(p) and len(p.C[1]) <= MAX_C_NNZ)
            if ps:
                return (op, (self.pick(ps),), dict(out=self.new_t(), transpose=self.chance(0.5)))
            ps = self.plans(lambda p: sm.dtname(p.A.dtype) == dtype)
            if ps:
                return ("spgemm", (self.pick(ps),), {})
            return self.r_plan_create(dtype)
        if not ts:
            return None
        if op == "ewise":
            pairs = [(i, j) for i in ts for j in ts if (self.m.t[i].rows, self.m.t[i].cols) == (self.m.t[j].rows, self.m.t[j].cols)]
            i, j = self.pick(pairs)
            return (op, (i, j), dict(out=self.new_t(), op=self.pick(ewiseref.OPS), pattern=self.pick(ewiseref.PATTERNS), alpha=self.pick(SCALES),
                                     beta=self.pick(SCALES)))
        i = self.pick(ts)
        T = self.m.t[i]
        if op == "select":
            sop = self.pick(selectref.POSITIONAL) if self.chance(0.6) else self.pick(selectref.OPS)
            thunk = float(self.rng.integers(-T.cols, T.cols + 1)) if sop in selectref.POSITIONAL else float(self.pick(VALUE_THUNKS))
            return (op, (i,), dict(out=self.new_t(), op=sop, thunk=thunk))
        if op == "sddmm":
            # S of either value type; the result holds the record's
            i = self.pick(self.tilings())
            return (op, (i,), dict(out=self.new_t(), dtype=dtype, semiring=self.pick(SEMIRINGS), k=self.sddmm_k(self.m.t[i]), **self.vals_args()))
        return ("save_load", (i,), dict(out=self.new_t()))

    def r_reader(self, dtype, tid=None, column=None):
        ts = [tid] if tid is not None else self.tilings(lambda T: sm.dtname(T.dtype) == dtype)
        if not ts:
            return None
        i = self.pick(ts)
        T = self.m.t[i]
        op = self.least(("mxv", "reduce", "spmm"), dtype)
        tr = self.chance(0.5) if column is None else column
        acc = self.chance(0.4)
        if op == "mxv":
            return (op, (i,), dict(semiring=self.pick(SEMIRINGS), transpose=tr, accumulate=acc, **self.vals_args()))
        if op == "reduce":
            return (op, (i,), dict(op=self.pick(ewiseref.OPS), dim="cols" if tr else "rows", accumulate=acc, seed=self.seed(), special=self.chance(0.25)))
        longest = int(np.diff(T.rp).max()) if T.nnz else 0
        ks = [k for k in SPMM_KS if k <= 17 or (longest <= 300 and max(T.rows, T.cols) * k <= 60_000)]   # (the numpy fold: one step per entry of the longest row, per column)
        return (op, (i,), dict(semiring=self.pick(SEMIRINGS), transpose=tr, k=int(self.pick(ks)), accumulate=acc, **self.vals_args()))

    def r_ctx(self, dtype):
        op = self.least(KINDS_CTX, None)
        return (op, (), dict(bytes=int(self.pick(RESERVES))) if op == "reserve" else {})

    def r_read_hot(self, dtype):
        """one of the four readers on the tiling written last: plan A side, plan B side, row walk, column walk"""
        i = self.hot
        if i not in self.m.t:
            return None
        T = self.m.t[i]
        w = T.last_writer
        how = self.least(("plan_a", "plan_b", "row", "col"), w)
        self.count[(how, w)] = self.count.get((how, w), 0) + 1
        if how in ("row", "col"):
            return self.r_reader(sm.dtname(T.dtype), i, how == "col")
        ps = self.plans(lambda p: (p.A if how == "plan_a" else p.B) is T)
        if ps:
            pid = self.pick(ps)
            return ("step3" if self.m.p[pid].state >= 2 and self.chance(0.5) else "spgemm", (pid,), {})
        # no plan reads it on that side yet: make one (and read on a later step)
        if len(self.m.p) >= MAX_PLANS:
            return self.r_plan_close(None)
        others = [j for j, B in self.m.t.items() if B.dtype == T.dtype and
                  ((T.cols == B.rows and self.m.products(T, B) <= MAX_PRODUCTS) if how == "plan_a" else (B.cols == T.rows and self.m.products(B, T) <= MAX_PRODUCTS))]
        if not others:
            return self.r_reader(sm.dtname(T.dtype), i)
        j = self.pick(others)
        self.count[(how, w)] -= 1
        return ("plan_create", (i, j, None) if how == "plan_a" else (j, i, None), dict(out=self.new_p(), complement=False, lo=0, hi=-1, semiring="plus_times"))

    # ---- deliberate refusals ---------------------------------------------------------------------------------------------------
    def r_refusal(self, dtype):
        m = self.m
        stale = self.plans(lambda p: not m.current(p))
        opts = []
        if stale:
            opts += ["export_not_current", "from_cplan_not_current"]
        cpl = [(i, T) for i, T in m.t.items() if T.prov is not None and T.prov[0] == "cplan" and T.nnz > 0]
        if [1 for i, T in cpl if T.prov[1] in m.p and not m.current(m.p[T.prov[1]])]:
            opts.append("refresh_plan_not_current")
        if [1 for i, T in cpl for q in m.p if q != T.prov[1] and m.current(m.p[q])]:
            opts.append("wrong_plan")
        ew = [(i, T) for i, T in m.t.items() if T.prov is not None and T.prov[0] == "ewise" and T.nnz > 0 and T.prov[1] in m.t and T.prov[2] in m.t]
        if ew:
            opts.append("wrong_ewise_source")
        se = [(i, T) for i, T in m.t.items() if T.prov is not None and T.prov[0] == "select" and T.nnz > 0 and T.prov[1] in m.t]
        if [1 for i, T in se if T.prov[2] in selectref.POSITIONAL] and len(m.t) >= 2:
            opts.append("wrong_select_source")
        if [1 for i, T in se if T.prov[2] not in selectref.POSITIONAL]:
            opts.append("select_by_value_refresh")
        if self.plans(lambda p: p.state < 2):
            opts.append("step_out_of_order")
        if self.plans(lambda p: p.M is not None):
            opts.append("masked_plan_option")
        if not opts:
            return None
        why = self.least(opts, "refusal")
        if why == "export_not_current":
            return (self.pick(("export_csr", "export_coo")), (self.pick(stale),), dict(expect=why))
        if why == "from_cplan_not_current":
            return ("from_cplan", (self.pick(stale),), dict(out=self.new_t(), transpose=self.chance(0.5), expect=why))
        if why == "refresh_plan_not_current":
            i, T = self.pick([(i, T) for i, T in cpl if T.prov[1] in m.p and not m.current(m.p[T.prov[1]])])
            return ("set_values_from_cplan", (i, T.prov[1]), dict(expect=why))
        if why == "wrong_plan":
            i, q = self.pick([(i, q) for i, T in cpl for q in m.p if q != T.prov[1] and m.current(m.p[q])])
            return ("set_values_from_cplan", (i, q), dict(expect=why))
        if why == "wrong_ewise_source":
            i, T = self.pick(ew)
            a, b = T.prov[1], T.prov[2]
            if a != b and self.chance(0.5):
                return ("set_values_from_ewise", (i, b, a), dict(expect=why))      # swapped operands
            other = [j for j in m.t if j != b]
            return ("set_values_from_ewise", (i, a, self.pick(other)), dict(expect=why)) if other else None
        if why == "wrong_select_source":
            i, T = self.pick([(i, T) for i, T in se if T.prov[2] in selectref.POSITIONAL])
            return ("set_values_from_select", (i, self.pick([j for j in m.t if j != T.prov[1]])), dict(expect=why))
        if why == "select_by_value_refresh":
            i, T = self.pick([(i, T) for i, T in se if T.prov[2] not in selectref.POSITIONAL])
            return ("set_values_from_select", (i, T.prov[1]), dict(expect=why))
        if why == "step_out_of_order":
            pid = self.pick(self.plans(lambda p: p.state < 2))
            return ("step2" if m.p[pid].state < 1 and self.chance(0.5) else "step3", (pid,), dict(expect=why))
        return ("set_option", (self.pick(self.plans(lambda p: p.M is not None)),), dict(name="wide", value=0, expect=why))

    # ---- the plan scenario: full pass, warm pass, option change, full pass, refresh of an operand, step 3 -----------------------------
    def start_scenario(self):
        ps = self.plans(lambda p: p.A.nnz > 0)
        if not ps:
            return
        pid = self.pick(ps)
        self.script = [("spgemm", pid), ("spgemm", pid), ("option", pid), ("spgemm", pid), ("refresh", pid), ("step3", pid)]
        self.scenarios += 1

    def r_script(self):
        what, pid = self.script[0]
        if pid not in self.m.p:
            self.script = []
            return None
        p = self.m.p[pid]
        if what == "step3" and p.state < 2:          # (something in between sent the plan back: catch up first)
            return ("step1" if p.state < 1 else "step2", (pid,), {})
        self.script.pop(0)
        if what == "option":
            name = self.pick([n for n in sorted(OPTION_VALUES) if not (p.M is not None and n == "wide")])
            vals = [v for v in OPTION_VALUES[name] if v != p.options[name]]
            return ("set_option", (pid,), dict(name=name, value=int(self.pick(vals))))
        if what == "refresh":
            tid = [i for i, T in self.m.t.items() if T is p.A][0]
            return (self.pick(("set_values", "set_values_device")), (tid,), dict(order=self.pick(("row", "col")), **self.vals_args()))
        return (what, (pid,), {})

    # ---- one step --------------------------------------------------------------------------------------------------------------
    def draw(self):
        dtype = self.want_dtype()
        if self.script and self.chance(0.5):
            return self.r_script()
        if not self.script and self.scenarios < 2 and self.m.p and self.chance(0.15):
            self.start_scenario()
        if len(self.m.t) < 2:
            return self.r_convert(dtype)
        if self.refusals * 12 < len(self.prog) and self.chance(0.09):
            return self.r_refusal(dtype)
        if self.chance(0.08):
            return self.r_chase(dtype)
        if self.hot is not None and self.chance(0.22):
            return self.r_read_hot(dtype)
        cat = self.pick(("convert", "plan_create", "plan_op", "writer", "derive", "reader", "ctx", "close", "plan_close", "export"),
                        (1.0, 0.5, 3.0, 2.3, 2.9, 0.3, 0.55, 0.3, 0.2, 0.45))
        return getattr(self, "r_" + cat)(dtype)

    def step(self):
        for _ in range(200):
            rec = self.draw()
            if rec is not None:
                break
        else:
            raise RuntimeError("the generator found no operation to emit")
        dtype = record_dtype(self.m, rec)
        res = self.m.apply(rec)
        assert (res.status != 0) == ("expect" in rec[2]), f"model and generator disagree on {rec}: status {res.status}"
        if res.status != 0:
            self.refusals += 1
            self.count[(rec[2]["expect"], "refusal")] = self.count.get((rec[2]["expect"], "refusal"), 0) + 1
        self.count[(rec[0], dtype)] = self.count.get((rec[0], dtype), 0) + 1
        if res.status == 0 and res.wrote in self.m.t and rec[0].startswith("set_values"):
            self.hot = res.wrote
        self.prog.append(rec)


class _Gen2(_Gen):
    """the second operation set: everything _Gen draws, plus the records listed in the module's docstring"""

    MAX_T = MAX_TILINGS2

    def __init__(self, seed):
        super().__init__(seed)
        self.turn = (int(seed) * 29) % (2 * len(KINDS2_T))   # where this program starts in the round of r_needy
        self.script2 = []                # pending steps of a scenario of the second set (see start_scenario2)
        self.cast = []                   # the tilings that scenario works on: not closed while it runs
        self.started = {}
        self.stalls = 0
        self.owed = None                 # the derivation a close made room for
        self.young = []                  # derived tilings not refreshed yet: half of them are refreshed soon

    def least(self, kinds, dtype):
        if tuple(kinds) == ("plan_a", "plan_b", "row", "col"):
            # the old readers of the tiling written last, after writer `dtype`: ties go round from a place every program has of its own,
            # so that the seed list as a whole follows every writer by every reader
            kinds = list(kinds)
            return min(kinds, key=lambda k: (self.count.get((k, dtype), 0), (kinds.index(k) - self.turn - len(str(dtype))) % 4))
        w = [BOOST2.get(k, BOOST.get(k, 1.0)) / (1 + self.count.get((k, dtype), 0)) ** 2 for k in kinds]
        return self.pick(kinds, w)

    def cycle(self, name, options):
        """one of `options`, those this program drew least under `name` first"""
        x = self.least(options, name)
        self.count[(x, name)] = self.count.get((x, name), 0) + 1
        return x

    # ---- the pool ----------------------------------------------------------------------------------------------------------
    def named(self, tid):
        T = self.m.t[tid]
        if tid in self.cast or any(T is p.A or T is p.B or T is p.M for p in self.m.p.values()):
            return True
        return any(tid in sm.sources(D.prov) for D in self.m.t.values())

    def of(self, dtype, pred=lambda T: True):
        return self.tilings(lambda T: sm.dtname(T.dtype) == dtype and pred(T))

    @staticmethod
    def solvable(T):
        return T.rows == T.cols and T.nnz <= MAX_TRSV_NNZ

    @staticmethod
    def factorable(T):
        return T.rows == T.cols and T.nnz <= MAX_TRSV_NNZ and sm.ilu0_cost(T) <= MAX_ILU0_COST and sm.missing_diag(T)[0] == 0

    def r_convert(self, dtype):
        """nearly half of the converted matrices are square and store their diagonal"""
        if len(self.m.t) >= self.MAX_T or not self.chance(0.55):
            return super().r_convert(dtype)
        return self.square_convert(dtype)

    def square_convert(self, dtype):
        op = self.least(("from_coo", "from_csr", "from_coo_device"), dtype)
        how = self.pick(("trsv", "ilu0", "randdiag"), (1.0, 1.0, 1.3))
        if how == "trsv":
            src = {"trsv": [self.pick(TRSV_CASES, TRSV_WEIGHT), int(self.chance(0.5))]}
        elif how == "ilu0":
            src = {"ilu0": self.pick(ILU0_CASES, ILU0_WEIGHT)}
        else:
            n = int(self.pick(DIMS))
            src = {"randdiag": [self.seed(), n, max(1, int(n * n * self.pick(DENSITIES)))]}
        return (op, (), dict(out=self.new_t(), src=src, dtype=dtype, transpose=op != "from_csr" and self.chance(0.3)))

    # ---- derivations: each takes the tiling to derive from (None: any of the value type) and returns a record or None ----------------
    def d_apply(self, dtype, i=None):
        ts = [i] if i is not None else self.of(dtype)
        if not ts:
            return None
        op = self.cycle("apply_op", applyref.OPS)
        thunk = float(self.cycle("powi_k", (1, 2, 64))) if op == "powi" else 0.0 if op in applyref.UNARY else float(self.pick(VALUE_THUNKS + (2.0,)))
        return ("apply", (self.pick(ts),), dict(out=self.new_t(), op=op, thunk=thunk))

    def scale_args(self):
        rows, cols = self.cycle("scale_vectors", ((True, False), (False, True), (True, True)))
        return dict(rows=self.seed() if rows else None, cols=self.seed() if cols else None, special=self.chance(0.25))

    def d_scale(self, dtype, i=None):
        ts = [i] if i is not None else self.of(dtype)
        if not ts:
            return None
        return ("scale", (self.pick(ts),), dict(out=self.new_t(), op=self.cycle("scale_op", applyref.BINOPS), **self.scale_args()))

    def region_spec(self, dim, n):
        """n different indices of 0 .. dim - 1 for assign: all of them in order where n == dim, a range, a host or a device list"""
        how = self.cycle("assign_list", ("all", "slice", "host", "device") if n == dim else ("slice", "host", "device"))
        if how == "all":
            return None
        if how == "slice":
            lo = int(self.rng.integers(0, dim - n + 1))
            return ["slice", lo, lo + n, 1]
        return [how, [int(x) for x in self.rng.permutation(dim)[:n]]]

    def d_assign(self, dtype, i=None):
        """C(I, J) = A with A any tiling of the pool that fits into C: where A stores less than C's region did, entries are deleted"""
        fits = lambda C, A: A.rows <= C.rows and A.cols <= C.cols and max(A.rows, A.cols) <= MAX_LIST and C.nnz + A.nnz <= MAX_C_NNZ // 2
        pairs = [(c, x) for c in ([i] if i is not None else self.of(dtype)) for x in self.of(sm.dtname(self.m.t[c].dtype))
                 if fits(self.m.t[c], self.m.t[x])]
        if not pairs:
            return None
        c, x = self.pick(pairs)
        C, A = self.m.t[c], self.m.t[x]
        accum = self.cycle("assign_accum", (None,) + applyref.BINOPS) if self.chance(0.5) else None
        return ("assign", (c, x), dict(out=self.new_t(), rows=self.region_spec(C.rows, A.rows), cols=self.region_spec(C.cols, A.cols), accum=accum))

    def d_build(self, dtype, i=None, op=None):
        """build / build_device from a small matrix's entries repeated; runs longer than the in-order limit only under the ops whose
        result does not depend on the grouping (the header lets plus and times round differently there)"""
        if self.chance(0.3):
            src = {"case": self.pick(("tiny_9x9", "rand_50", "ragged_37", "dense_tile", "empty_rows"))}
        else:
            rows, cols = int(self.pick(DIMS)), int(self.pick(DIMS))
            src = {"rand": [self.seed(), rows, cols, min(3000, max(1, int(rows * cols * self.pick(DENSITIES)))), False]}
        dup = self.cycle("dup", buildref.DUP_OPS)
        op = op or self.least(("build", "build_device"), dtype)
        return (op, (), dict(out=self.new_t(), dtype=dtype, src=src, dup=dup, transpose=self.chance(0.3), keep_map=self.chance(0.6),
                             lens_seed=self.seed(), long=dup not in ("plus", "times") and self.chance(0.5)))

    def d_build_device(self, dtype, i=None):
        return self.d_build(dtype, op="build_device")

    def sampled_operands(self, s, fixed=None):
        """(a, b, transpose_b) with A . B (or A . B^T) of S's shape, of one value type (fixed: that of an in-place target)"""
        S = self.m.t[s]
        out = []
        for a, A in self.m.t.items():
            if A.rows != S.rows or (fixed is not None and (A.dtype != fixed or a == s)):
                continue
            if S.nnz and int(np.diff(A.rp)[sm.rows_of(S.rows, S.rp)].sum()) > MAX_SAMPLED_WORK:
                continue
            for b, B in self.m.t.items():
                if B.dtype == A.dtype and not (fixed is not None and b == s):
                    out += [(a, b, tb) for tb in (False, True) if ((B.cols, B.rows) if tb else (B.rows, B.cols)) == (A.cols, S.cols)]
        return out

    def d_sampled_mxm(self, dtype, i=None):
        cand = [(s,) + x for s in self.tilings() for x in self.sampled_operands(s) if sm.dtname(self.m.t[x[0]].dtype) == dtype]
        if not cand:
            return None
        s, a, b, tb = self.pick(cand)
        return ("sampled_mxm", (s, a, b), dict(out=self.new_t(), dtype=dtype, semiring=self.cycle("sampled_semiring", sorted(SEMIRINGS)), transpose_b=tb))

    def r_sampled_writer(self, dtype):
        cand = [(t,) + x for t in self.of(dtype, lambda T: T.nnz > 0) for x in self.sampled_operands(t, self.m.t[t].dtype)]
        if not cand:
            return None
        t, a, b, tb = self.pick(cand)
        semiring = self.cycle("sampled_semiring", sorted(SEMIRINGS))
        # (an accumulate under plus_pair adds a tile pair's count in one addition: only exact on small integers, so it is left out)
        return ("set_values_sampled_mxm", (t, a, b), dict(semiring=semiring, transpose_b=tb, accumulate=semiring != "plus_pair" and self.chance(0.5)))

    def d_select_topk(self, dtype, i=None):
        ts = [i] if i is not None else self.of(dtype)
        if not ts:
            return None
        i = self.pick(ts)
        T = self.m.t[i]
        dim = self.cycle("topk_dim", topkref.DIMS)
        longest = int(np.bincount(T.ci, minlength=1).max() if dim == "cols" else np.diff(T.rp).max()) if T.nnz else 0
        k = self.cycle("topk_k", ("0", "1", "line", "beyond"))
        k = {"0": 0, "1": 1, "line": longest, "beyond": longest + int(self.pick((1, 1000)))}[k]
        return ("select_topk", (i,), dict(out=self.new_t(), k=int(k), order=self.cycle("topk_order", topkref.ORDERS), dim=dim))

    def d_transpose(self, dtype, i=None):
        ts = [i] if i is not None else self.of(dtype)
        return ("transpose", (self.pick(ts),), dict(out=self.new_t())) if ts else None

    def index_spec(self, dim, keep_all=False):
        how = "all" if keep_all else self.cycle("extract_list", ("all", "slice", "host", "device"))
        if how == "all":
            return None
        if how == "slice":
            lo = int(self.rng.integers(0, dim))
            return ["slice", lo, int(self.rng.integers(lo + 1, dim + 1)), int(self.pick((1, 1, 2)))]
        n = min(int(self.pick((1, dim // 2 + 1, dim + 3))), MAX_LIST)
        return [how, [int(x) for x in self.rng.integers(0, dim, n)]]     # (out of order, with repeats)

    def d_extract(self, dtype, i=None):
        ts = [i] if i is not None else self.of(dtype, lambda T: T.nnz <= MAX_C_NNZ // 4)
        if not ts:
            return None
        i = self.pick(ts)
        T = self.m.t[i]
        if self.chance(0.2):                 # a piece of T.split(row_sizes, col_sizes): what split emits is one extract per piece
            spec = []
            for dim in (T.rows, T.cols):
                cuts = sorted({0, dim, int(self.rng.integers(0, dim + 1))})
                k = int(self.rng.integers(0, len(cuts) - 1))
                spec.append(["slice", cuts[k], cuts[k + 1], 1])
            return ("extract", (i,), dict(out=self.new_t(), rows=spec[0], cols=spec[1]))
        return ("extract", (i,), dict(out=self.new_t(), rows=self.index_spec(T.rows), cols=self.index_spec(T.cols)))

    def d_kron(self, dtype, i=None):
        fits = lambda A, B: A.nnz * B.nnz <= MAX_KRON_NNZ and A.rows * B.rows <= 3 * MAX_DIM2 and A.cols * B.cols <= 3 * MAX_DIM2
        pairs = [(x, y) for x in ([i] if i is not None else self.of(dtype)) for y in self.of(sm.dtname(self.m.t[x].dtype))
                 if fits(self.m.t[x], self.m.t[y])]
        if not pairs and i is None:          # (no two tilings of this value type are small enough: convert a small one)
            rows, cols = int(self.pick((1, 9, 16))), int(self.pick((1, 9, 16)))
            src = {"rand": [self.seed(), rows, cols, int(self.rng.integers(1, rows * cols + 1)), False]}
            return (self.least(("from_coo", "from_csr", "from_coo_device"), dtype), (), dict(out=self.new_t(), src=src, dtype=dtype, transpose=False))
        if not pairs:
            return None
        same = [p for p in pairs if p[0] == p[1]]
        x, y = self.pick(same) if same and self.chance(0.3) else self.pick(pairs)
        return ("kron", (x, y), dict(out=self.new_t(), op=self.cycle("kron_op", kronref.BINOPS)))

    def d_concat(self, dtype, i=None):
        ts = [i] if i is not None else self.of(dtype)
        if not ts:
            return None
        i = self.pick(ts)
        T = self.m.t[i]
        dtype = sm.dtname(T.dtype)
        rowmates = self.of(dtype, lambda U: U.rows == T.rows)
        colmates = self.of(dtype, lambda U: U.cols == T.cols)
        shape = self.cycle("concat_shape", CONCAT_SHAPES)
        if shape == "1xn":
            grid = [[i] + [self.pick(rowmates) for _ in range(int(self.pick((1, 2))))]]
        elif shape == "nx1":
            grid = [[i]] + [[self.pick(colmates)] for _ in range(int(self.pick((1, 2))))]
        elif shape == "2x2":
            b, c = self.pick(rowmates), self.pick(colmates)
            fit = self.of(dtype, lambda U: (U.rows, U.cols) == (self.m.t[c].rows, self.m.t[b].cols))
            grid = [[i, b], [c, self.pick(fit) if fit else None]]
        elif shape == "none_cell":
            grid = [[i, None], [None, self.pick(self.of(dtype))]]
        elif shape == "same_twice":
            grid = [[i, i]] if self.chance(0.5) else [[i], [i]]
        else:                            # a strip of no rows (or no columns), given by its size alone
            grid = [[i], [None]] if self.chance(0.5) else [[i, None]]
        cells = [[None if h is None else self.m.t[h] for h in row] for row in grid]
        rs = [next((c.rows for c in row if c is not None), 0) for row in cells]
        cs = [next((row[k].cols for row in cells if row[k] is not None), 0) for k in range(len(grid[0]))]
        if sum(rs) > MAX_DIM2 or sum(cs) > MAX_DIM2 or sum(c.nnz for row in cells for c in row if c is not None) > MAX_CONCAT_NNZ:
            return None
        return ("concat", tuple(h for row in grid for h in row),
                dict(out=self.new_t(), dtype=dtype, grid=[len(grid), len(grid[0])], row_sizes=[int(x) for x in rs], col_sizes=[int(x) for x in cs]))

    def d_ilu0(self, dtype, i=None):
        ts = [i] if i is not None and self.factorable(self.m.t[i]) else [] if i is not None else self.of(dtype, self.factorable)
        if not ts and i is None:             # (nothing of this value type can be factored: convert something that can)
            return self.square_convert(dtype)
        return ("ilu0", (self.pick(ts),), dict(out=self.new_t())) if ts else None

    def r_derive(self, dtype):
        if len(self.m.t) >= self.MAX_T:
            return self.r_close(dtype)
        if self.chance(0.12):
            return super().r_derive(dtype)
        # the kind this program derived least in this value type that the pool allows (ties at random)
        # (ilu0 and kron fit few pools: they count half)
        kinds = list(sm.KINDS2 + ("select_topk", "build", "build_device", "sampled_mxm"))
        used = {k: self.count.get((k, dtype), 0) / (3 if k == "kron" else 2 if k == "ilu0" else 1) for k in kinds}
        for k in sorted(kinds, key=lambda k: (used[k], self.rng.random())):
            rec = getattr(self, "d_" + k)(dtype)
            if rec is not None:
                return rec
        return None

    # ---- refreshes -----------------------------------------------------------------------------------------------------------
    def refresh_rec(self, i):
        """the set_values_from_<kind> record of a tiling of the second set's kinds, None while a source is gone"""
        T = self.m.t[i]
        if T.prov is not None and T.prov[0] == "build":
            return ("set_values_from_build", (i,), {"build": T.prov[2]}) if T.prov[1]["keep_map"] and T.nnz else None
        if T.prov is None or T.prov[0] not in sm.KINDS2 or T.nnz == 0 or not all(s in self.m.t for s in sm.sources(T.prov)):
            return None
        tail = tuple(T.prov[1]) if T.prov[0] == "concat" else sm.sources(T.prov)
        return ("set_values_from_" + T.prov[0], (i,) + tail, {"scale": True} if T.prov[0] == "scale" else {})

    def emit(self, rec):
        """a refresh record as it is emitted: a scale's vectors are given anew"""
        if rec is not None and rec[0] == "set_values_from_scale" and "scale" in rec[2]:
            return (rec[0], rec[1], dict(self.scale_args(), **{k: v for k, v in rec[2].items() if k != "scale"}))
        if rec is not None and rec[0] == "set_values_from_build" and "build" in rec[2]:
            return (rec[0], rec[1], dict(self.vals_args(), nnz_in=rec[2]["build"]))
        return rec

    def r_chase(self, dtype):
        cand = []
        for i, T in self.m.t.items():
            if T.prov is None or T.nnz == 0:
                continue
            k = T.prov[0]
            if k in sm.KINDS2 + ("build",):
                ok = self.refresh_rec(i) is not None
            elif k == "cplan":
                ok = T.prov[1] in self.m.p
            else:
                ok = T.prov[1] in self.m.t and (T.prov[2] in self.m.t if k == "ewise" else T.prov[2] in selectref.POSITIONAL)
            if ok:
                cand.append((self.count.get(("set_values_from_" + k, sm.dtname(T.dtype)), 0), i))
        if not cand:
            return None
        low = min(c for c, _ in cand)
        i = self.pick([i for c, i in cand if c == low])
        return self.emit(self.refresh_rec(i)) or _Gen.r_writer(self, None, i, refresh=True)

    def r_writer(self, dtype, tid=None, refresh=False):
        ts = [tid] if tid is not None else self.of(dtype)
        recs = [r for r in (self.refresh_rec(i) for i in ts) if r]
        if tid is None and self.chance(0.2):
            rec = self.r_sampled_writer(dtype)
            if rec:
                return rec
        if recs and (self.chance(0.4) or (refresh and self.m.t[tid].prov[0] in sm.KINDS2)):
            op = self.least(sorted({r[0] for r in recs}), dtype)
            return self.emit(self.pick([r for r in recs if r[0] == op]))
        return super().r_writer(dtype, tid, refresh)

    # ---- readers ---------------------------------------------------------------------------------------------------------------
    def solve_rec(self, i, uplo=None):
        T = self.m.t[i]
        unit = bool(sm.missing_diag(T)[0]) or self.chance(0.4)
        return ("trsv", (i,), dict(uplo=uplo or self.cycle("uplo", ("lower", "upper")), unit_diag=unit, in_place=self.chance(0.5), **self.vals_args()))

    def r_needy(self, dtype):
        """the (kind, value type) of the second set this program ran least, the first the pool allows.  Ties go by a fixed round
        over all of them that every program enters at a place of its own (self.turn), so that the seed list as a whole reaches
        every one about equally often -- a random tie-break left some short of the ten times tests/test_seq_cpu.py asks for"""
        cells = [(k, d) for k in KINDS2_T for d in ("f64", "f32")]
        order = sorted(range(len(cells)), key=lambda c: (self.count.get(cells[c], 0), (c - self.turn) % len(cells)))
        for c in order[:16]:
            k, dtype = cells[c]
            rec = None
            if k.startswith("set_values_from_"):
                recs = [r for r in (self.refresh_rec(i) for i in self.of(dtype)) if r and r[0] == k]
                if recs:
                    return self.emit(self.pick(recs))
                k = k[16:]                   # (nothing of that kind is alive: derive one, the refresh comes on a later draw)
            elif k in ("lu_solve", "ilu0_info") and not [1 for i in self.of(dtype, self.solvable) if (self.m.t[i].prov or ("",))[0] == "ilu0"]:
                k = "ilu0"
            if k == "set_values_sampled_mxm":
                rec = self.r_sampled_writer(dtype)
            elif k in ("mxv_frontier", "mxv_arg", "reduce_arg"):
                rec = self.r_fold(dtype, force=k)
            elif k in ("trsv", "trsv_info", "bfs", "bfs_parents", "lu_solve", "ilu0_info", "triangle_count"):
                rec = self.r_solve(dtype, force=k)
                if rec is None and k == "triangle_count":
                    return self.r_triangles(dtype)
            elif len(self.m.t) >= self.MAX_T:
                self.owed = (k, dtype)       # (make room now, derive on the next draw)
                return self.r_close(dtype)
            else:
                rec = getattr(self, "d_" + k)(dtype)
            if rec is not None:
                return rec
        return None

    def r_triangles(self, dtype):
        """triangle_count on a symmetric pattern of this value type; where none is alive, make room, convert one, count on the next draw"""
        rec = self.r_solve(dtype, force="triangle_count")
        if rec is None:
            self.owed = ("triangle_count", dtype)
            if len(self.m.t) >= self.MAX_T:
                return self.r_close(dtype)
            src = {"ilu0": self.pick(("dense_15", "dense_17", "dense_33", "tridiagonal_200", "band_100_20", "double_arrow_400"))}
            rec = (self.least(("from_coo", "from_csr", "from_coo_device"), dtype), (), dict(out=self.new_t(), src=src, dtype=dtype, transpose=False))
        return rec

    def r_solve(self, dtype, tid=None, force=None):
        ts = [i for i in ([tid] if tid is not None else self.of(dtype)) if self.solvable(self.m.t[i])]
        if not ts:
            return None
        factors = [i for i in ts if self.m.t[i].prov is not None and self.m.t[i].prov[0] == "ilu0"]
        op = self.least(("trsv", "trsv_info", "bfs", "bfs_parents") + (("lu_solve", "ilu0_info") if factors else ()), sm.dtname(self.m.t[ts[0]].dtype))
        graphs = [i for i in ts if self.m.t[i].rows <= 700 and sm.symmetric(self.m.t[i])]
        if force is None and graphs and self.chance(0.15):
            op = "triangle_count"
        if force is not None:
            if (force in ("lu_solve", "ilu0_info") and not factors) or (force == "triangle_count" and not graphs):
                return None
            op = force
        if op == "triangle_count":
            return (op, (self.pick(graphs),), {})
        if op in ("bfs", "bfs_parents"):
            i = self.pick(ts)
            return (op, (i,), dict(source=int(self.rng.integers(0, self.m.t[i].rows)), transpose=self.chance(0.5)))
        if op == "trsv":
            return self.solve_rec(self.pick(ts))
        if op == "trsv_info":
            return (op, (self.pick(ts),), dict(uplo=self.cycle("uplo", ("lower", "upper"))))
        return (op, (self.pick(factors),), self.vals_args() if op == "lu_solve" else {})

    def r_factor_read(self):
        """lu_solve or ilu0_info on a live factor, the value type that saw fewer first"""
        fs = [i for i, T in self.m.t.items() if T.prov is not None and T.prov[0] == "ilu0"]
        if not fs:
            return None
        i = self.pick(fs, [1.0 / (1 + self.count.get(("lu_solve", sm.dtname(self.m.t[i].dtype)), 0)) ** 2 for i in fs])
        op = self.least(("lu_solve", "ilu0_info"), sm.dtname(self.m.t[i].dtype))
        return (op, (i,), self.vals_args() if op == "lu_solve" else {})

    def r_fold(self, dtype, tid=None, column=None, arg=None, force=None):
        """mxv_frontier, mxv_arg or reduce_arg (arg: None any, False the first, True one of the other two)"""
        ts = [tid] if tid is not None else self.of(dtype, lambda T: T.nnz <= MAX_TRSV_NNZ)
        if not ts:
            return None
        i = self.pick(ts)
        op = self.least({None: ("mxv_frontier", "mxv_arg", "reduce_arg"), False: ("mxv_frontier",), True: ("mxv_arg", "reduce_arg")}[arg],
                        sm.dtname(self.m.t[i].dtype))
        op = force or op
        tr = self.chance(0.5) if column is None else column
        if op == "reduce_arg":
            return (op, (i,), dict(op=self.cycle("arg_op", ("min", "max")), dim="cols" if tr else "rows"))
        a = dict(transpose=tr, x_present=self.cycle("x_present", ("none", "sparse", "empty")), mask=self.cycle("mask", (None, "mask", "complement")),
                 out_present=self.chance(0.5), accumulate=self.chance(0.4), **self.vals_args())
        if op == "mxv_arg":
            kind = self.cycle("arg_kind", argref.KINDS)
            return (op, (i,), dict(a, kind=kind, x_none=kind in argref.INDEX_KINDS and self.chance(0.5)))
        semiring = "plus_pair" if self.chance(0.15) else self.pick(SEMIRINGS)
        return (op, (i,), dict(a, semiring=semiring, x_none=semiring == "plus_pair" and self.chance(0.6)))

    def r_reader(self, dtype, tid=None, column=None):
        if column is None and self.chance(0.7):
            rec = self.r_solve(dtype, tid) if self.chance(0.65) else self.r_fold(dtype, tid)
            if rec:
                return rec
        return super().r_reader(dtype, tid, column)

    def r_read_hot(self, dtype):
        """the solves count among the readers of the tiling written last"""
        i = self.hot
        if i in self.m.t and self.solvable(self.m.t[i]) and self.chance(0.1):
            w = self.m.t[i].last_writer
            how = self.least(("trsv_lower", "trsv_upper"), w)
            self.count[(how, w)] = self.count.get((how, w), 0) + 1
            return self.solve_rec(i, how[5:])
        if i in self.m.t and self.m.t[i].nnz <= MAX_TRSV_NNZ and self.chance(0.1):
            w = self.m.t[i].last_writer
            how = self.least(("frontier_row", "frontier_col", "arg_row", "arg_col"), w)
            self.count[(how, w)] = self.count.get((how, w), 0) + 1
            return self.r_fold(dtype, i, how.endswith("col"), how.startswith("arg"))
        return super().r_read_hot(dtype)

    # ---- deliberate refusals -----------------------------------------------------------------------------------------------------
    def r_refusal(self, dtype):
        if self.chance(0.25):
            return super().r_refusal(dtype)
        m = self.m
        derived = [i for i, T in m.t.items() if T.prov is not None and T.nnz > 0]
        fresh = [i for i in m.t if self.refresh_rec(i)]
        concats = [i for i in fresh if m.t[i].prov[0] == "concat"]
        oblong = [i for i, T in m.t.items() if T.rows != T.cols]
        holed = [i for i, T in m.t.items() if T.rows == T.cols and sm.missing_diag(T)[0] and T.nnz <= MAX_TRSV_NNZ]
        opts = ["powi_thunk", "extract_empty_device"]
        regions = [(c, x) for c, C in m.t.items() for x, A in m.t.items() if C.dtype == A.dtype and 2 <= A.rows <= min(C.rows, MAX_LIST)
                   and A.cols <= C.cols and C.nnz + A.nnz <= MAX_C_NNZ // 2]
        opts += ["assign_repeat_device"] if regions else []
        built = [i for i, T in m.t.items() if T.prov is not None and T.prov[0] == "build" and T.nnz > 0]
        opts += ["build_refresh_no_map"] if [i for i in built if not m.t[i].prov[1]["keep_map"]] else []
        opts += ["build_refresh_wrong_nnz"] if [i for i in built if m.t[i].prov[1]["keep_map"]] else []
        opts += ["wrong_kind_refresh"] if derived else []
        opts += ["wrong_source_refresh"] if [i for i in fresh if m.t[i].prov[0] not in ("concat", "build")] and len(m.t) >= 3 else []
        opts += ["concat_wrong_count"] if concats else []
        opts += ["concat_swapped"] if [i for i in concats if len(set(m.t[i].prov[1])) > 1] else []
        opts += ["trsv_nonsquare", "ilu0_nonsquare"] if oblong else []
        opts += ["trsv_missing_diag", "ilu0_missing_diag"] if holed else []
        opts += ["trsv_overlap"] if [i for i, T in m.t.items() if self.solvable(T) and T.rows >= 2] else []
        why = self.least(opts, "refusal")
        if why == "powi_thunk":
            return ("apply", (self.pick(self.tilings()),), dict(out=self.new_t(), op="powi", thunk=float(self.pick((0, 65, -1, 2.5))), expect=why))
        if why == "extract_empty_device":
            i = self.pick(self.tilings())
            T = m.t[i]
            rows, cols = (["device", []], self.index_spec(T.cols)) if self.chance(0.5) else (self.index_spec(T.rows), ["device", []])
            return ("extract", (i,), dict(out=self.new_t(), rows=rows, cols=cols, expect=why))
        if why in ("build_refresh_no_map", "build_refresh_wrong_nnz"):
            i = self.pick([i for i in built if m.t[i].prov[1]["keep_map"] == (why == "build_refresh_wrong_nnz")])
            n = m.t[i].prov[2] + (0 if why == "build_refresh_no_map" else int(self.pick((-1, 1))))
            return ("set_values_from_build", (i,), dict(self.vals_args(), nnz_in=n, expect=why))
        if why == "assign_repeat_device":
            c, x = self.pick(regions)
            C, A = m.t[c], m.t[x]
            rows = [int(r) for r in self.rng.permutation(C.rows)[:A.rows]]
            rows[int(self.rng.integers(1, len(rows)))] = rows[0]
            cols = None if A.cols == C.cols else ["slice", 0, A.cols, 1]
            return ("assign", (c, x), dict(out=self.new_t(), rows=["device", rows], cols=cols, accum=None, expect=why))
        if why == "wrong_kind_refresh":
            i = self.pick(derived)
            T = m.t[i]
            kind = self.pick([k for k in ("apply", "transpose", "extract", "ilu0") if k != T.prov[0]])
            alive = [s for s in sm.sources(T.prov) if s in m.t]
            return ("set_values_from_" + kind, (i, alive[0] if alive else self.pick([j for j in m.t if j != i] or [i])), dict(expect=why))
        if why == "wrong_source_refresh":
            op, ids, _ = self.refresh_rec(self.pick([i for i in fresh if m.t[i].prov[0] not in ("concat", "build")]))
            k = int(self.rng.integers(1, len(ids)))
            other = [j for j in m.t if j != ids[k]]
            ids = ids[:k] + (self.pick(other),) + ids[k + 1:]
            return self.emit((op, ids, dict(_, expect=why)))
        if why == "concat_wrong_count":
            op, ids, _ = self.refresh_rec(self.pick(concats))
            return (op, ids[:-1] if len(ids) > 2 and self.chance(0.5) else ids + (ids[-1],), dict(expect=why))
        if why == "concat_swapped":
            op, ids, _ = self.refresh_rec(self.pick([i for i in concats if len(set(m.t[i].prov[1])) > 1]))
            x, y = self.pick([(x, y) for x in range(1, len(ids)) for y in range(x + 1, len(ids)) if ids[x] != ids[y]])
            ids = list(ids)
            ids[x], ids[y] = ids[y], ids[x]
            return (op, tuple(ids), dict(expect=why))
        if why in ("trsv_nonsquare", "trsv_missing_diag"):
            i = self.pick(oblong if why == "trsv_nonsquare" else holed)
            return ("trsv", (i,), dict(uplo=self.pick(("lower", "upper")), unit_diag=why == "trsv_nonsquare" and self.chance(0.5), in_place=self.chance(0.5),
                                       expect=why, **self.vals_args()))
        if why in ("ilu0_nonsquare", "ilu0_missing_diag"):
            return ("ilu0", (self.pick(oblong if why == "ilu0_nonsquare" else holed),), dict(out=self.new_t(), expect=why))
        rec = self.solve_rec(self.pick([i for i, T in m.t.items() if self.solvable(T) and T.rows >= 2]))
        return (rec[0], rec[1], dict(rec[2], in_place=False, overlap=True, expect=why))

    # ---- scenarios of the second set: a chain refreshed link by link, the life of a factor, a concat between refreshes ---------------------
    def start_scenario2(self):
        kinds = [k for k in ("chain", "life", "concat") if self.started.get(k, 0) < (2 if k == "chain" else 1)]
        if not kinds or len(self.m.t) > self.MAX_T - 1:
            return
        # the life of a factor and the concat need one free place, the chain three; what this program has not run comes first
        kind = "life" if "life" in kinds else self.pick(kinds)
        if kind == "chain" and len(self.m.t) > self.MAX_T - 3:
            return
        small = lambda T: 0 < T.nnz <= 3000 and max(T.rows, T.cols) <= 700
        if kind == "chain":
            ts = self.tilings(lambda T: small(T) and self.factorable(T)) if self.chance(0.6) else []
            ts = ts or self.tilings(small)
            steps = ["link", "link", "link", "colread", "write", "refresh1", "refresh2", "refresh3", "read"]
        elif kind == "life":
            ts = self.tilings(lambda T: T.nnz > 0 and self.factorable(T))
            steps = ["ilu0", "lu_solve", "write", "refresh1", "lu_solve"]
        else:
            ts = self.tilings(small)
            steps = ["concat", "refresh1", "write", "refresh1", "ctx", "refresh1"]
        if ts:
            self.cast, self.script2, self.stalls = [self.pick(ts)], steps, 0
            self.started[kind] = self.started.get(kind, 0) + 1

    def r_script2(self, dtype):
        if any(i not in self.m.t or self.m.t[i].nnz == 0 for i in self.cast) or self.stalls > 8:
            self.script2, self.cast = [], []
            return None
        what = self.script2[0]
        base, tip = self.cast[0], self.cast[-1]
        dtype = sm.dtname(self.m.t[base].dtype)
        if what in ("link", "ilu0", "concat"):
            if len(self.m.t) >= self.MAX_T:
                self.stalls += 1
                return self.r_close(dtype)
            if what == "link":
                kinds = list(sm.KINDS2)
                rec = None
                while kinds and rec is None:
                    k = self.least(kinds, "link")
                    kinds.remove(k)
                    rec = self.d_extract_all(tip) if k == "extract" else getattr(self, "d_" + k)(dtype, tip)
                if rec is not None:
                    self.count[(rec[0], "link")] = self.count.get((rec[0], "link"), 0) + 1
            else:
                rec = getattr(self, "d_" + what)(dtype, tip)
            if rec is None:
                self.script2, self.cast = [], []
                return None
            self.cast.append(rec[2]["out"])
        elif what == "write":
            rec = (self.pick(("set_values", "set_values_device")), (base,), dict(order=self.pick(("row", "col")), **self.vals_args()))
        elif what.startswith("refresh"):
            rec = self.emit(self.refresh_rec(self.cast[int(what[7:])]))
        elif what == "ctx":
            rec = ("trim", (), {}) if self.chance(0.5) else ("reserve", (), dict(bytes=int(self.pick(RESERVES))))
        elif what == "lu_solve":
            rec = ("lu_solve", (tip,), self.vals_args())
        elif what == "colread":
            rec = _Gen.r_reader(self, dtype, self.pick(self.cast[1:]), True)
        else:
            rec = _Gen.r_reader(self, dtype, tip)
        if rec is None:
            self.script2, self.cast = [], []
            return None
        self.script2 = self.script2[1:]
        if not self.script2:
            self.cast = []
        return rec

    def d_extract_all(self, i):
        """a link of a chain: an extract that keeps every row and takes the columns as they are or by a slice"""
        T = self.m.t[i]
        return ("extract", (i,), dict(out=self.new_t(), rows=None, cols=None if self.chance(0.5) else ["slice", 0, T.cols, 1]))

    def step(self):
        super().step()
        op, _, a = self.prog[-1]
        if "expect" not in a and (op in sm.KINDS2 or (op.startswith("build") and a["keep_map"])) and self.chance(0.5):
            self.young.append(a["out"])

    def draw(self):
        dtype = self.want_dtype()
        if self.script and self.chance(0.5):
            return self.r_script()
        if self.script2 and self.chance(0.6):
            return self.r_script2(dtype)
        if self.owed is not None:
            (k, d), self.owed = self.owed, None
            rec = self.r_triangles(d) if k == "triangle_count" else getattr(self, "d_" + k)(d) if len(self.m.t) < self.MAX_T else None
            if rec is not None:
                return rec
        if self.young and self.chance(0.3):
            i = self.young.pop(0)
            rec = self.emit(self.refresh_rec(i)) if i in self.m.t else None
            if rec is not None:
                return rec
        if not self.script and self.scenarios < 1 and self.m.p and self.chance(0.15):
            self.start_scenario()
        if not self.script2 and len(self.m.t) >= 2 and self.chance(0.2):
            self.start_scenario2()
        if len(self.m.t) < 2:
            return self.r_convert(dtype)
        if self.refusals * 12 < len(self.prog) and self.chance(0.09):
            return self.r_refusal(dtype)
        if self.chance(0.08):
            return self.r_chase(dtype)
        if self.chance(0.03):
            return self.r_factor_read()
        if self.chance(0.1):                 # the first set's derivations, so that the new readers and refreshes meet their writers too
            return _Gen.r_derive(self, dtype)
        if self.hot is not None and self.chance(0.45):
            return self.r_read_hot(dtype)
        if self.chance(0.8):
            return self.r_needy(dtype)
        cat = self.pick(("convert", "plan_create", "plan_op", "writer", "derive", "reader", "ctx", "close", "plan_close", "export"),
                        (1.0, 0.4, 1.0, 1.6, 5.0, 1.4, 0.5, 0.3, 0.2, 0.3))
        return getattr(self, "r_" + cat)(dtype)


class _Gen3(_Gen2):
    """the third operation set: everything _Gen2 draws, plus the graph routines, the solvers and the hierarchies"""

    def __init__(self, seed):
        super().__init__(seed)
        self.nk = self.nh = 0
        self.turn3 = (int(seed) * 13) % (2 * len(KINDS3_T))
        self.script3, self.cast3, self.kind3, self.stalls3 = [], {}, None, 0
        self.started3, self.args3 = {}, None
        self.sched_by = {}             # tiling -> who built its column schedule ("reader" / "graph")
        self.last_graph = None           # the kind of the last graph call
        self.after_trim = False          # a trim ran and no graph call since

    # ---- the pools -------------------------------------------------------------------------------------------------------------
    def named(self, tid):
        if tid in self.cast3.values() or any(tid in (K.a, K.pre) for K in self.m.k.values()) or any(tid == H.a for H in self.m.h.values()):
            return True
        return super().named(tid)

    def held(self, hid):
        """a live solver names this hierarchy, or a scenario works on it"""
        return hid in self.cast3.values() or any(K.pre == hid for K in self.m.k.values())

    def new_k(self):
        self.nk += 1
        return f"k{self.nk}"

    def new_h(self):
        self.nh += 1
        return f"h{self.nh}"

    def system_convert(self, dtype, graph=False):
        op = self.least(("from_coo", "from_csr", "from_coo_device"), dtype)
        src = {"graph": self.pick(GRAPH_SOURCES)} if graph else {"system": self.pick(SYSTEMS, SYSTEM_WEIGHT)}
        return (op, (), dict(out=self.new_t(), src=src, dtype=dtype, transpose=False))

    def square_convert(self, dtype):
        """a third of the square matrices are the Krylov / multigrid tests' systems, some the colouring tests' graphs"""
        x = self.rng.random()
        return self.system_convert(dtype, graph=x < 0.1) if x < 0.45 else super().square_convert(dtype)

    def room(self, dtype):
        """a record that makes room for a new tiling, or None where there is room"""
        return self.r_close(dtype) if len(self.m.t) >= self.MAX_T else None

    # ---- graph routines ----------------------------------------------------------------------------------------------------------
    @staticmethod
    def graphable(T):
        return T.rows == T.cols and T.nnz <= MAX_GRAPH_NNZ and T.rows <= MAX_DIM2

    def graph_args(self, kind, T, name):
        sym = sm.symmetric(T) and self.chance(0.3)
        a = dict(symmetric=sym)
        if kind in ("colour", "mis", "aggregate") or (kind == "colour_order" and self.cycle("order_of", ("colour", "components")) == "colour"):
            p = self.cycle("prio_" + kind, PRIORITIES).split("_")
            a["prio"] = ["seed", int(p[1])] if p[0] == "seed" else p
        if kind == "colour_order":
            a["of"] = "colour" if "prio" in a else "components"
        elif kind == "components":
            a["ids"] = self.cycle("cc_ids", (True, False))
        elif kind == "mis":
            a["distance"] = self.cycle("mis_distance", (1, 2))
        elif kind == "aggregate":
            a["roots"] = self.cycle("agg_roots", (True, False))
        return a

    def sched_state(self, i):
        return self.sched_by.get(i, "none") if "mx_cols" in self.m.t[i].built else "none"

    def n_graph(self, dtype, kind, i=None):
        ts = [i] if i is not None else self.of(dtype, self.graphable)
        if not ts:
            return self.room(dtype) or self.square_convert(dtype)
        prov = lambda j: (self.m.t[j].prov or ("plain",))[0]
        w = [1.0 / ((1 + self.count.get((kind, self.sched_state(j)), 0)) ** 2 * (1 + self.count.get((kind, prov(j)), 0)) ** 2
                    * (1 + self.count.get(("graph", prov(j)), 0))) for j in ts]
        i = self.pick(ts, w)
        a = self.graph_args(kind, self.m.t[i], kind)
        if not a["symmetric"]:
            self.count[(kind, self.sched_state(i))] = self.count.get((kind, self.sched_state(i)), 0) + 1
        for k in (kind, "graph"):
            self.count[(k, prov(i))] = self.count.get((k, prov(i)), 0) + 1
        return (kind, (i,), a)

    def r_provenance(self, dtype):
        """an owed draw, as r_needy's: a graph routine on a tiling of a provenance no graph routine of this program has met -- or,
        where none is alive, a step towards one (the third set's own kinds leave the second set's derivations fewer draws)"""
        missing = [k for k in sm.KINDS2 + ("cplan",) if not self.count.get(("graph", k), 0)]
        if not missing:
            return None
        kind = missing[(self.turn3 + len(missing)) % len(missing)]
        alive = [i for i in self.tilings(self.graphable) if (self.m.t[i].prov or ("",))[0] == kind]
        if alive:
            return self.n_graph(dtype, self.next_graph_kind() if self.last_graph else "colour", self.pick(alive))
        if len(self.m.t) >= self.MAX_T:
            return self.r_close(dtype)
        squares = self.of(dtype, lambda T: self.graphable(T) and T.nnz <= 3000 and T.rows <= 700)
        if kind == "cplan":
            ps = self.plans(lambda p: p.A.rows == p.B.cols and self.graphable(p.A))
            cur = [i for i in ps if self.m.current(self.m.p[i]) and len(self.m.p[i].C[1]) <= MAX_GRAPH_NNZ]
            if cur:
                return ("from_cplan", (self.pick(cur),), dict(out=self.new_t(), transpose=self.chance(0.5)))
            if ps:
                return ("spgemm", (self.pick(ps),), {})
            if len(self.m.p) >= MAX_PLANS:
                return self.r_plan_close(dtype)
            squares = [i for i in squares if self.m.products(self.m.t[i], self.m.t[i]) <= MAX_PRODUCTS // 4]
            return ("plan_create", (i := self.pick(squares), i, None), dict(out=self.new_p(), complement=False, lo=0, hi=-1, semiring="plus_times")) \
                if squares else None
        if kind == "kron":
            small = self.of(dtype, lambda T: T.rows == T.cols and T.rows <= 48 and T.nnz <= 150)
            if not small:
                n = int(self.pick((9, 16)))
                return (self.least(("from_coo", "from_csr", "from_coo_device"), dtype), (),
                        dict(out=self.new_t(), src={"randdiag": [self.seed(), n, 2 * n]}, dtype=dtype, transpose=False))
            return ("kron", (self.pick(small), self.pick(small)), dict(out=self.new_t(), op=self.cycle("kron_op", kronref.BINOPS)))
        if not squares:
            return None
        i = self.pick(squares)
        if kind == "concat":
            return ("concat", (i, None, None, i), dict(out=self.new_t(), dtype=sm.dtname(self.m.t[i].dtype), grid=[2, 2],
                                                      row_sizes=[self.m.t[i].rows] * 2, col_sizes=[self.m.t[i].cols] * 2))
        if kind == "extract":
            return self.d_extract_all(i)
        if kind == "assign":
            return ("assign", (i, i), dict(out=self.new_t(), rows=None, cols=None, accum=self.cycle("assign_accum", (None,) + applyref.BINOPS)))
        return getattr(self, "d_" + kind)(dtype, i)

    def next_graph_kind(self):
        """the graph routine that followed the last one least (or, after a trim, that ran first after one least)"""
        key = "after_trim" if self.after_trim else self.last_graph
        kinds = [k for k in GRAPH_KINDS if k != key]
        return min(kinds, key=lambda k: (self.count.get(((k, key), "after"), 0), self.rng.random()))

    # ---- solvers -------------------------------------------------------------------------------------------------------------------
    def system_ok(self, T, max_iters=1):
        return T.rows == T.cols and T.nnz > 0 and T.nnz * max(max_iters, 1) <= MAX_SOLVE_WORK

    def amg_ok(self, T):
        return T.rows == T.cols and 0 < T.nnz <= MAX_AMG_NNZ and sm.ilu0_cost(T) <= MAX_AMG_PRODUCTS and sm.missing_diag(T)[0] == 0

    def solver_opts(self, nnz, fnnz=0):
        its = [k for k in MAX_ITERS3 if nnz * max(k, 1) <= MAX_SOLVE_WORK and fnnz * max(k, 1) <= MAX_LU_WORK] or [0]
        max_iters = int(self.cycle("max_iters", its))
        every = self.cycle("check_every", ("1", "3", "8", "above"))
        return dict(max_iters=max_iters, check_every=max_iters + 5 if every == "above" else int(every), rtol=self.pick(RTOLS), atol=self.pick(ATOLS))

    def n_krylov_create(self, dtype, a=None, pair=None, pre=None):
        if len(self.m.k) >= MAX_SOLVERS:
            return self.n_krylov_close(dtype, force=True)
        method, pc = pair or self.cycle("method_precond", [f"{m} {p}" for m, p in METHOD_PRECOND]).split()
        ts = [a] if a is not None else self.of(dtype, self.system_ok)
        if pc == "amg" and pre is None:
            hs = [(h, H.a) for h, H in self.m.h.items() if H.a in ts]
            if not hs:
                return self.n_amg_create(dtype)
            pre, a = self.pick(hs)
        elif pc == "lu" and pre is None:
            fs = [(f, F.prov[1]) for f, F in self.m.t.items() if F.prov is not None and F.prov[0] == "ilu0" and F.prov[1] in ts and self.solvable(F)]
            if not fs:
                cand = [i for i in ts if self.factorable(self.m.t[i])]
                return self.room(dtype) or (("ilu0", (self.pick(cand),), dict(out=self.new_t())) if cand else self.system_convert(dtype))
            pre, a = self.pick(fs)
        elif a is None:
            if not ts:
                return self.room(dtype) or self.system_convert(dtype)
            shared = [i for i in ts if any(K.a == i for K in self.m.k.values())]
            a = self.pick(shared) if shared and self.chance(0.35) else self.pick(ts, [1.0 / (1 + self.m.t[i].nnz) ** 0.5 for i in ts])
        A = self.m.t[a]
        opts = self.solver_opts(A.nnz, self.m.t[pre].nnz if pc == "lu" else 3 * A.nnz if pc == "amg" else 0)
        return ("krylov_create", (a, pre), dict(out=self.new_k(), method=method, precond=pc, **opts))

    def solve_args(self):
        return dict(x0=self.cycle("x0", (True, False)), history=self.cycle("history", (True, False)), seed=self.seed(), special=self.chance(0.15))

    def n_krylov_solve(self, dtype, k=None):
        ks = [k] if k is not None else [k for k, K in self.m.k.items() if sm.dtname(self.m.t[K.a].dtype) == dtype]
        if not ks:
            return self.n_krylov_create(dtype)
        # the solver that solved least, those whose A, factor or hierarchy changed since first
        return ("krylov_solve", (min(ks, key=lambda k: (len(self.m.k[k].trail), self.rng.random())),), self.solve_args())

    def n_krylov_close(self, dtype, force=False):
        ks = [k for k, K in self.m.k.items() if k not in self.cast3.values() and (force or sm.dtname(self.m.t[K.a].dtype) == dtype)]
        ks = [k for k in ks if self.m.k[k].trail] or ([] if not force else ks)      # (a solver that never solved is closed last)
        return ("krylov_close", (self.pick(ks),), {}) if ks else None

    def n_tiled_solve(self, dtype):
        pc = self.cycle("tiled_precond", ("none", "ilu0"))
        ts = self.of(dtype, lambda T: self.system_ok(T) and (pc == "none" or (self.factorable(T) and len(self.m.t) < self.MAX_T)))
        if not ts:
            return self.room(dtype) or self.system_convert(dtype)
        a = self.pick(ts)
        opts = self.solver_opts(self.m.t[a].nnz, self.m.t[a].nnz if pc == "ilu0" else 0)
        return ("tiled_solve", (a,), dict(method=self.cycle("tiled_method", ("cg", "bicgstab")), precond=pc, **opts, **self.solve_args()))

    # ---- hierarchies -----------------------------------------------------------------------------------------------------------------
    def n_amg_create(self, dtype, a=None, refreshable=None):
        if len(self.m.h) >= MAX_HIERARCHIES:
            return self.n_amg_close(dtype, force=True)
        ts = [a] if a is not None else self.of(dtype, self.amg_ok)
        if not ts:
            return self.room(dtype) or self.system_convert(dtype)
        a = self.pick(ts)
        sweeps, coarse_sweeps = self.cycle("amg_sweeps", AMG_SWEEPS)
        if refreshable is None:
            refreshable = self.cycle("refreshable", (1, 0, 1))
        return ("amg_create", (a,), dict(out=self.new_h(), smooth=int(self.cycle("amg_smooth", AMG_SMOOTH)), coarse_size=int(self.cycle("amg_coarse", AMG_COARSE)),
                                         sweeps=int(sweeps), coarse_sweeps=int(coarse_sweeps), symmetric=bool(sm.symmetric(self.m.t[a]) and self.chance(0.6)),
                                         refreshable=int(refreshable)))

    def hierarchies(self, dtype, pred=lambda H: True):
        return [h for h, H in self.m.h.items() if sm.dtname(self.m.t[H.a].dtype) == dtype and pred(H)]

    def n_amg_refresh(self, dtype):
        hs = self.hierarchies(dtype, lambda H: H.opts["refreshable"])
        return ("amg_refresh", (self.pick(hs),), {}) if hs else self.n_amg_create(dtype, refreshable=1)

    def n_amg_apply(self, dtype):
        hs = self.hierarchies(dtype)
        return ("amg_apply", (self.pick(hs),), self.vals_args()) if hs else self.n_amg_create(dtype)

    def n_amg_info(self, dtype):
        hs = self.hierarchies(dtype)
        return ("amg_info", (self.pick(hs),), {}) if hs else self.n_amg_create(dtype)

    def n_amg_level(self, dtype):
        hs = self.hierarchies(dtype)
        if not hs:
            return self.n_amg_create(dtype)
        h = self.pick(hs)
        H = self.m.h[h]
        which = self.cycle("level_which", ("A", "P", "R"))
        if len(H.levels) == 1:
            which = "A"
        level = int(self.rng.integers(0, len(H.levels) - (which != "A")))
        T = self.m.level_tiling(H, level, which)
        what = self.cycle("level_reader", ("mxv", "reduce", "export_csr", "graph") if which == "A" and self.graphable(T) else ("mxv", "reduce", "export_csr"))
        if what == "graph":
            what = self.cycle("level_graph", ("colour", "components", "mis", "aggregate"))
            args = self.graph_args(what, T, what)
        elif what == "export_csr":
            args = {}
        else:
            tr, acc = self.chance(0.5), self.chance(0.4)
            args = dict(semiring=self.pick(SEMIRINGS), transpose=tr, accumulate=acc, **self.vals_args()) if what == "mxv" else \
                dict(op=self.pick(ewiseref.OPS), dim="cols" if tr else "rows", accumulate=acc, **self.vals_args())
        return ("amg_level", (h,), dict(level=level, which=which, reader=[what, args]))

    def n_amg_close(self, dtype, force=False):
        hs = [h for h in (self.m.h if force else self.hierarchies(dtype)) if not self.held(h)]
        if hs:
            return ("amg_close", (self.pick(hs),), {})
        return self.n_krylov_close(dtype, force=True) if force else None

    def r_needy3(self, dtype):
        """r_needy over the third set's kinds: the (kind, value type) this program ran least (a solve counts a third), the first the
        pool allows; ties go round from a place every program has of its own"""
        cells = [(k, d) for k in KINDS3_T for d in ("f64", "f32")]
        order = sorted(range(len(cells)), key=lambda c: (self.count.get(cells[c], 0) / NEEDY3_SHARE.get(cells[c][0], 1.0), (c - self.turn3) % len(cells)))
        for c in order[:10]:
            k, d = cells[c]
            if k in GRAPH_KINDS:
                # the routine the round asks for; where the order of the graph calls has a gap, the one that fills it
                rec = self.n_graph(d, self.next_graph_kind() if self.last_graph and self.chance(0.5) else k)
            else:
                rec = getattr(self, "n_" + k)(d)
            if rec is not None:
                return rec
        return None

    # ---- deliberate refusals ---------------------------------------------------------------------------------------------------------
    def r_refusal(self, dtype):
        if self.chance(0.45):
            return super().r_refusal(dtype)
        m = self.m
        oblong = [i for i, T in m.t.items() if T.rows != T.cols]
        square = [i for i, T in m.t.items() if self.graphable(T)]
        systems = [i for i, T in m.t.items() if self.system_ok(T)]
        holed = [i for i, T in m.t.items() if T.rows == T.cols and sm.missing_diag(T)[0] and T.nnz <= MAX_AMG_NNZ]
        diag = lambda T: T.rows == T.cols and sm.missing_diag(T)[0] == 0 and T.nnz <= MAX_TRSV_NNZ
        factors = [(i, f) for i in systems for f, F in m.t.items() if diag(F) and F.rows == m.t[i].rows]
        same = [(i, f) for i, f in factors if m.t[f].dtype == m.t[i].dtype]
        other = [(i, f) for i, f in factors if m.t[f].dtype != m.t[i].dtype]
        foreign = [(i, h) for h, H in m.h.items() for i in systems if i != H.a and m.t[i].dtype == m.t[H.a].dtype]
        fixed = [h for h, H in m.h.items() if not H.opts["refreshable"]]
        single = [k for k, K in m.k.items() if m.t[K.a].dtype == np.float32]
        opts = ["colour_nonsquare", "components_nonsquare", "mis_nonsquare", "aggregate_nonsquare", "krylov_nonsquare"] if oblong else []
        opts += ["mis_distance_3", "priority_overlap"] if square else []
        opts += ["lu_no_factor"] if systems else []
        opts += ["factor_other_precond"] if same else []
        opts += ["factor_other_dtype"] if other else []
        opts += ["amg_other_matrix"] if foreign else []
        opts += ["amg_missing_diag"] if holed else []
        opts += ["refresh_not_refreshable"] if fixed else []
        opts += ["solve_wrong_form"] if single else []
        if not opts:
            return super().r_refusal(dtype)
        why = self.least(opts, "refusal")
        plain = dict(symmetric=False, expect=why)
        kopts = dict(max_iters=5, check_every=8, rtol=1e-8, atol=0.0, expect=why)
        if why.endswith("_nonsquare") and why != "krylov_nonsquare":
            kind = why[:-10]
            extra = dict(colour=dict(prio=["seed", 0]), components=dict(ids=True), mis=dict(prio=["seed", 0], distance=2), aggregate=dict(prio=["seed", 0], roots=True))
            return (kind, (self.pick(oblong),), dict(plain, **extra[kind]))
        if why == "krylov_nonsquare":
            return ("krylov_create", (self.pick(oblong), None), dict(kopts, out=self.new_k(), method=self.pick(("cg", "bicgstab")), precond="none"))
        if why == "mis_distance_3":
            return ("mis", (self.pick(square),), dict(plain, prio=["seed", 0], distance=3))
        if why == "priority_overlap":
            return ("colour", (self.pick(square),), dict(plain, prio=[self.pick(("equal", "ties")), "device"], overlap=True))
        if why == "lu_no_factor":
            return ("krylov_create", (self.pick(systems), None), dict(kopts, out=self.new_k(), method=self.pick(("cg", "bicgstab")), precond="lu"))
        if why in ("factor_other_precond", "factor_other_dtype"):
            i, f = self.pick(same if why == "factor_other_precond" else other)
            pc = self.pick(("none", "diag")) if why == "factor_other_precond" else "lu"
            return ("krylov_create", (i, f), dict(kopts, out=self.new_k(), method=self.pick(("cg", "bicgstab")), precond=pc))
        if why == "amg_other_matrix":
            i, h = self.pick(foreign)
            return ("krylov_create", (i, h), dict(kopts, out=self.new_k(), method=self.pick(("cg", "bicgstab")), precond="amg"))
        if why == "amg_missing_diag":
            return ("amg_create", (self.pick(holed),), dict(out=self.new_h(), smooth=1, coarse_size=8, sweeps=1, coarse_sweeps=4, symmetric=False,
                                                           refreshable=1, expect=why))
        if why == "refresh_not_refreshable":
            return ("amg_refresh", (self.pick(fixed),), dict(expect=why))
        return ("krylov_solve", (self.pick(single),), dict(self.solve_args(), wrong_form=True, expect=why))

    # ---- scenarios of the third set: the life of a solver, the life of a hierarchy, the reorder ------------------------------------------
    SCRIPTS3 = dict(solver=("ilu0", "create_lu", "solve", "write", "refresh_factor", "solve", "graph_other", "solve"),
                    hierarchy=("amg_create", "create_amg", "solve", "write", "amg_refresh", "solve", "ctx", "amg_apply", "amg_refresh", "amg_info"),
                    reorder=("colour", "colour_order", "extract", "ilu0", "trsv_info", "create_lu", "solve"))

    def start_scenario3(self):
        kinds = [k for k in SCRIPTS3_ORDER if self.started3.get(k, 0) < 1]
        if not kinds:
            return
        kind = kinds[(self.turn3 + len(self.prog)) % len(kinds)]
        small = lambda T: T.nnz > 0 and self.factorable(T) and T.nnz * 30 <= MAX_LU_WORK
        if kind == "solver":
            ts = self.tilings(small)
        elif kind == "hierarchy":
            ts = self.tilings(lambda T: self.amg_ok(T) and T.nnz * 3 * 8 <= MAX_LU_WORK * 4)
        else:
            ts = self.tilings(lambda T: small(T) and T.rows <= MAX_LIST)
        if ts:
            self.kind3, self.script3, self.cast3, self.stalls3 = kind, list(self.SCRIPTS3[kind]), {"A": self.pick(ts)}, 0
            self.started3[kind] = self.started3.get(kind, 0) + 1

    def end_scenario3(self):
        self.script3, self.cast3, self.kind3 = [], {}, None
        return None

    def r_script3(self, dtype):
        c, m = self.cast3, self.m
        if any((v not in m.t and v not in m.k and v not in m.h) for v in c.values()) or self.stalls3 > 10:
            return self.end_scenario3()
        what = self.script3[0]
        base = c.get("R", c["A"])            # (the reorder's later steps work on the reordered matrix)
        dtype = sm.dtname(m.t[c["A"]].dtype)
        rec = None
        if what in ("ilu0", "extract") and len(m.t) >= self.MAX_T:
            self.stalls3 += 1
            return self.r_close(dtype)
        if what in ("create_lu", "create_amg") and len(m.k) >= MAX_SOLVERS:
            self.stalls3 += 1
            return self.n_krylov_close(dtype, force=True)
        if what == "amg_create" and len(m.h) >= MAX_HIERARCHIES:
            self.stalls3 += 1
            return self.n_amg_close(dtype, force=True)
        if what == "ilu0":
            rec = ("ilu0", (base,), dict(out=self.new_t()))
            c["F"] = rec[2]["out"]
        elif what in ("create_lu", "create_amg"):
            pair = (self.cycle("scenario_method", ("cg", "bicgstab")), what[7:])
            rec = self.n_krylov_create(dtype, a=base, pair=pair, pre=c["F"] if what == "create_lu" else c["H"])
            c["K"] = rec[2]["out"]
        elif what == "solve":
            rec = ("krylov_solve", (c["K"],), self.solve_args())
        elif what == "write":
            rec = _Gen.r_writer(self, None, c["A"])
        elif what == "refresh_factor":
            rec = ("set_values_from_ilu0", (c["F"], base), {})
        elif what == "graph_other":
            others = [i for i in self.of(dtype, self.graphable) + self.tilings(self.graphable) if i not in c.values()]
            if not others:
                self.stalls3 += 1
                return self.room(dtype) or self.square_convert(dtype)
            rec = self.n_graph(dtype, self.next_graph_kind() if self.last_graph else "colour", others[0] if self.chance(0.5) else self.pick(others))
        elif what == "amg_create":
            rec = self.n_amg_create(dtype, a=c["A"], refreshable=1)
            c["H"] = rec[2]["out"]
        elif what in ("amg_refresh", "amg_info"):
            rec = (what, (c["H"],), {})
        elif what == "amg_apply":
            rec = (what, (c["H"],), self.vals_args())
        elif what == "ctx":
            rec = ("trim", (), {}) if self.cycle("scenario_ctx", ("trim", "reserve")) == "trim" else ("reserve", (), dict(bytes=int(self.pick(RESERVES))))
        elif what == "colour":
            p = self.cycle("prio_colour", PRIORITIES).split("_")
            self.args3 = dict(symmetric=False, prio=["seed", int(p[1])] if p[0] == "seed" else p)
            rec = ("colour", (base,), dict(self.args3))
        elif what == "colour_order":
            rec = ("colour_order", (base,), dict(self.args3, of="colour"))
        elif what == "extract":              # the permutation as both lists, as Tiled.reorder_by_colour hands it to extract
            perm = [int(v) for v in m.apply(("colour_order", (base,), dict(self.args3, of="colour"))).out[1]]
            rec = ("extract", (base,), dict(out=self.new_t(), rows=["device", perm], cols=["device", perm]))
            c["R"] = rec[2]["out"]
        elif what == "trsv_info":
            rec = ("trsv_info", (c["F"],), dict(uplo=self.cycle("uplo", ("lower", "upper"))))
        if rec is None:
            return self.end_scenario3()
        self.script3 = self.script3[1:]
        if not self.script3:
            self.count[(self.kind3, "scenario3")] = self.count.get((self.kind3, "scenario3"), 0) + 1
            self.end_scenario3()
        return rec

    def step(self):
        before = {i: "mx_cols" in T.built for i, T in self.m.t.items()}
        super().step()
        op, ids, a = self.prog[-1]
        if "expect" in a:
            return
        for i, T in self.m.t.items():
            if "mx_cols" in T.built and not before.get(i, False):
                self.sched_by[i] = "graph" if op in GRAPH_KINDS else "amg" if op == "amg_create" else "reader"
        if op in GRAPH_KINDS:
            key = "after_trim" if self.after_trim else self.last_graph
            self.count[((op, key), "after")] = self.count.get(((op, key), "after"), 0) + 1
            self.last_graph, self.after_trim = op, False
        elif op == "trim":
            self.after_trim = True

    def draw(self):
        dtype = self.want_dtype()
        if self.script3 and self.chance(0.55):
            return self.r_script3(dtype)
        if not self.script3 and not self.script2 and len(self.m.t) >= 2 and self.chance(0.3):
            self.start_scenario3()
        if len(self.m.t) >= 2 and not self.script and not self.script2:
            if self.after_trim and self.chance(0.6):
                return self.n_graph(dtype, self.next_graph_kind())
            if self.refusals * 12 < len(self.prog) and self.chance(0.06):
                return self.r_refusal(dtype)
            if self.chance(0.06):
                rec = self.r_provenance(dtype)
                if rec is not None:
                    return rec
            hot =self.hot if self.hot in self.m.t else None
            if hot is not None and self.chance(0.3):     # what holds the tiling written last reads it next
                ks = [k for k, K in self.m.k.items() if hot in (K.a, K.pre)]
                hs = [h for h, H in self.m.h.items() if H.a == hot and H.opts["refreshable"]]
                if hs and self.chance(0.5):
                    return ("amg_refresh", (self.pick(hs),), {})
                if ks:
                    return self.n_krylov_solve(dtype, self.pick(ks))
            if self.chance(0.62):
                return self.r_needy3(dtype)
        return super().draw()


SCRIPTS3_ORDER = ("solver", "hierarchy", "reorder")


def op_set(seed):
    """the operation set a seed draws from: the second from SET2_FROM on, the third from SET3_FROM on"""
    return 3 if int(seed) >= SET3_FROM else 2 if int(seed) >= SET2_FROM else 1


def context_kind(seed):
    """the context kind a committed seed runs on (any other seed: by its value)"""
    for seeds in (SEEDS2, SEEDS3):
        if seed in seeds:
            return CONTEXT_KINDS[seeds.index(seed) % 3]
    return CONTEXT_KINDS[(SEEDS.index(seed) if seed in SEEDS else int(seed)) % 3]


def program(seed, steps):
    g = {1: _Gen, 2: _Gen2, 3: _Gen3}[op_set(seed)](int(seed))
    while len(g.prog) < steps:
        g.step()
    return g.prog
