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
"""
import json

import numpy as np

import ewiseref
import selectref
import seqmodel as sm
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
    return sm.dtname(model.p[h].A.dtype if h in model.p else model.t[h].dtype)


class _Gen:
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
        if len(self.m.t) >= MAX_TILINGS:
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
            if len(p.C[1]) <= MAX_C_NNZ and len(self.m.t) < MAX_TILINGS:
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
        if len(self.m.t) >= MAX_TILINGS:
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


def context_kind(seed):
    """the context kind a committed seed runs on (any other seed: by its value)"""
    return CONTEXT_KINDS[(SEEDS.index(seed) if seed in SEEDS else int(seed)) % 3]


def program(seed, steps):
    g = _Gen(int(seed))
    while len(g.prog) < steps:
        g.step()
    return g.prog
