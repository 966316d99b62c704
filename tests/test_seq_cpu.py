"""CPU: what the sequence test (tests/seqgen.py, tests/seqmodel.py, tests/test_gpu_seq.py) can check without a GPU.

  - program(seed, steps) is a pure function of its arguments and its text form round-trips;
  - the model alone executes every committed program, every record is well-typed, none is skipped;
  - the model's plan results agree with oracle.Plan (the tiled restatement: another route than the model's oracle.csr_spgemm /
    semiringref) at every spgemm step: this guards the model's glue, the references have their own CPU tests;
  - the coverage conditions the committed seed list must meet (test_coverage_conditions).  They are conditions, not measurements:
    if a change to the generator misses one, change the weights or add seeds.

The programs of the second operation set (sg.SEEDS2) have their own walk, table and conditions (test_second_set_coverage_conditions),
those of the third (sg.SEEDS3) theirs (walk3, table3, test_third_set_coverage_conditions), and the first two sets' programs are
pinned by their digests.

One condition is read narrower than it could be: each derivation map (C^T's, ewise's, select's) can only be built by its own
set_values_from_* entry point, so "first built by two different operation kinds" cannot hold for it; asserted instead is that each
is built at least twice and at least once on a tiling that already holds another lazily built structure.
"""
import collections
import hashlib
import json
import os

import numpy as np
import pytest

import concatref
import seqgen as sg
import seqmodel as sm

WRITERS = ("set_values_row", "set_values_col", "from_cplan", "from_ewise", "from_select", "sddmm", "sddmm_acc")
READERS = ("plan_a", "plan_b", "row", "col")
SCENARIO = ("full", "warm", "option", "full", "refresh", "step3")
LAZY = ("vmap_row", "vmap_col", "vmap_t", "mx_cols")
MAPS = ("map_cplan", "map_ewise", "map_select")

_PROGRAMS = {}


def _program(seed):
    if seed not in _PROGRAMS:
        _PROGRAMS[seed] = sg.program(seed, sg.STEPS)
    return _PROGRAMS[seed]


def _has_subsequence(trail, want):
    it = iter(trail)
    return all(any(x == w for x in it) for w in want)


def walk(prog, cov, kind, oracle=None):
    """run the model over one program, collecting the coverage figures; with an oracle, check every spgemm step's C against
    oracle.Plan"""
    m = sm.Model()
    trails = []
    for i, rec in enumerate(prog):
        op, ids, a = rec
        dtype = sg.record_dtype(m, rec)
        for h in ids:
            assert h is None or h in m.t or h in m.p or h in m.k or h in m.h, f"step {i}: {rec} names a handle that is not alive"
        built = {h: set(m.t[h].built) for h in ids if h in m.t}
        if op in ("mxv", "reduce", "spmm"):
            col = a["transpose"] if op != "reduce" else a["dim"] == "cols"
            reads = [(m.t[ids[0]].last_writer, "col" if col else "row")]
        elif op in ("step3", "spgemm"):
            reads = [(m.p[ids[0]].A.last_writer, "plan_a"), (m.p[ids[0]].B.last_writer, "plan_b")]
        else:
            reads = []
        if op == "plan_close":
            trails.append(m.p[ids[0]].trail)
        res = m.apply(rec)
        assert (res.status != 0) == ("expect" in a), f"step {i}: {rec}: model status {res.status}"
        cov["steps"] += 1
        if res.status != 0:
            cov["refusals"][a["expect"]] += 1
            continue
        cov["ops"][(op, dtype)] += 1
        for w, r in reads:
            if w is not None:
                cov["pairs"][(w, r)] += 1
        for h, before in built.items():
            if h in m.t:
                for s in m.t[h].built - before:
                    cov["first"][s].add(op)
                    if s in MAPS:
                        cov["maps"][s].append(bool(before))
        if oracle is not None and op == "spgemm":
            _check_against_oracle_plan(oracle, m.p[ids[0]], f"step {i}: {rec}")
    trails += [p.trail for p in m.p.values()]
    if any(_has_subsequence(t, SCENARIO) for t in trails):
        cov["scenario"][kind] += 1


def _check_against_oracle_plan(oracle, p, label):
    A, B = p.A, p.B
    oa = oracle.Tiled(A.rows, A.cols, sm.rows_of(A.rows, A.rp), A.ci, A.vals.astype(np.float64))
    ob = oracle.Tiled(B.rows, B.cols, sm.rows_of(B.rows, B.rp), B.ci, B.vals.astype(np.float64))
    rp, ci, v = oracle.Plan(oa, ob, p.lo, p.hi, f32=A.dtype == np.float32).export_csr()
    rows = p.row0 + sm.rows_of(len(rp) - 1, rp)
    if p.M is not None:
        mi, mj, _ = p.M.coo()
        keep = np.isin(rows * B.cols + ci, mi * B.cols + mj) != p.complement
        rows, ci, v = rows[keep], ci[keep], v[keep]
    mrp, mci, mv = p.C
    assert np.array_equal(p.row0 + sm.rows_of(len(mrp) - 1, mrp), rows) and np.array_equal(mci, ci), f"{label}: structure"
    if p.semiring == "plus_times":
        v = v.astype(A.dtype)
        assert sm.same(v, mv), f"{label}: values"


def coverage(oracle=None, seeds=sg.SEEDS):
    cov = dict(steps=0, ops=collections.Counter(), pairs=collections.Counter(), refusals=collections.Counter(),
               first=collections.defaultdict(set), maps=collections.defaultdict(list), scenario=collections.Counter())
    for seed in seeds:
        walk(_program(seed), cov, sg.context_kind(seed), oracle)
    return cov


def table(cov):
    lines = [f"sequence test coverage: {len(sg.SEEDS)} seeds x {sg.STEPS} steps = {cov['steps']} steps, "
             f"{sum(cov['refusals'].values())} deliberate refusals"]
    lines.append("operation kind            f64   f32")
    for k in sg.KINDS_T + sg.KINDS_P:
        lines.append(f"  {k:24s}{cov['ops'][(k, 'f64')]:5d} {cov['ops'][(k, 'f32')]:5d}")
    lines += [f"  {k:24s}{cov['ops'][(k, None)]:5d}" for k in sg.KINDS_CTX]
    lines.append("writer -> reader          " + " ".join(f"{r:>7s}" for r in READERS))
    for w in WRITERS:
        lines.append(f"  {w:24s}" + " ".join(f"{cov['pairs'][(w, r)]:7d}" for r in READERS))
    lines.append("first built by")
    lines += [f"  {s:24s}{', '.join(sorted(cov['first'][s]))}" for s in LAZY + MAPS]
    lines.append("refusals                  " + ", ".join(f"{k} {cov['refusals'][k]}" for k in sg.REFUSALS))
    lines.append("plan scenario seen on     " + ", ".join(f"{k}: {cov['scenario'][k]} programs" for k in sg.CONTEXT_KINDS))
    return "\n".join(lines)


def test_program_is_a_pure_function_and_its_text_round_trips():
    for seed in (sg.SEEDS[0], sg.SEEDS[7], 5):
        a, b = sg.program(seed, 60), sg.program(seed, 60)
        assert a == b
        assert sg.loads(sg.dumps(a)) == a
        assert sg.program(seed, 30) == a[:30]          # a longer program extends a shorter one
    assert sg.program(1, 40) != sg.program(2, 40)
    assert len(sg.SEEDS) == len(set(sg.SEEDS)) and len(sg.SEEDS) % 3 == 0
    assert [sg.context_kind(s) for s in sg.SEEDS[:3]] == list(sg.CONTEXT_KINDS)


def test_model_runs_every_committed_program_and_agrees_with_the_tiled_oracle(oracle):
    """every record is well-typed and none is skipped (walk asserts both); at every spgemm step C equals oracle.Plan's"""
    for seeds in (sg.SEEDS, sg.SEEDS3):          # (the third set's programs hold plans too: the same check of every spgemm step)
        cov = coverage(oracle, seeds)
        assert cov["steps"] == len(seeds) * sg.STEPS
        assert sum(cov["ops"].values()) + sum(cov["refusals"].values()) == cov["steps"]


def test_coverage_conditions():
    cov = coverage()
    print("\n" + table(cov))
    # every operation kind at least 20 times, in both value types
    for k in sg.KINDS_T + sg.KINDS_P:
        for d in ("f64", "f32"):
            assert cov["ops"][(k, d)] >= 20, f"{k} in {d}: {cov['ops'][(k, d)]} times"
    for k in sg.KINDS_CTX:
        assert cov["ops"][(k, None)] >= 20, k
    # every (value writer -> reader kind) pair on one handle
    for w in WRITERS:
        for r in READERS:
            assert cov["pairs"][(w, r)] >= 1, f"{w} -> {r}"
    # lazily built structures: first built by at least two different operation kinds
    for s in LAZY:
        assert len(cov["first"][s]) >= 2, f"{s}: first built only by {sorted(cov['first'][s])}"
    for s in MAPS:
        assert len(cov["maps"][s]) >= 2 and any(cov["maps"][s]), f"{s}: built {len(cov['maps'][s])} times"
    # full pass -> warm pass -> option change -> full pass -> refresh of an operand -> step 3, on every context kind
    for k in sg.CONTEXT_KINDS:
        assert cov["scenario"][k] >= 1, k
    # refusals
    assert sum(cov["refusals"].values()) * 10 <= cov["steps"]
    for k in sg.REFUSALS:
        assert cov["refusals"][k] >= 3, f"refusal {k}: {cov['refusals'][k]} times"


# ---- the second operation set (sg.SEEDS2) ---------------------------------------------------------------------------------------
DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seq_program_digests.json")
WRITERS2 = tuple("from_" + k for k in sm.KINDS2) + ("from_build", "sampled", "sampled_acc")
READERS2 = ("sampled_operand", "frontier_row", "frontier_col", "arg_row", "arg_col", "trsv_lower", "trsv_upper")
MAPS2 = ("map_transpose", "map_extract", "map_assign", "map_kron", "map_concat", "map_build")
SCHEDULES = ("trsv_lower", "trsv_upper")
LIFE = ("ilu0", "lu_solve", "source", "refresh", "lu_solve")
CONCAT_LIFE = ("refresh", "source", "refresh", "ctx", "refresh")


def test_the_first_sets_programs_are_those_of_the_commit_that_added_them():
    """SHA-256 of the text form of every program of SEEDS, recorded before the second set was added, and of SEEDS2, recorded
    before the third was"""
    want = json.load(open(DIGESTS))
    assert sorted(want) == sorted(str(s) for s in sg.SEEDS + sg.SEEDS2)
    for seed in sg.SEEDS + sg.SEEDS2:
        assert hashlib.sha256(sg.dumps(_program(seed)).encode()).hexdigest() == want[str(seed)], f"seed {seed}: the program changed"


def _downstream(m, tid):
    """the tilings derived from tid, transitively"""
    out, grew = {tid}, True
    while grew:
        grew = False
        for j, D in m.t.items():
            if j not in out and any(s in out for s in sm.sources(D.prov)):
                out.add(j)
                grew = True
    return out - {tid}


def _same_tiling(a, b):
    return (a.rows, a.cols) == (b.rows, b.cols) and np.array_equal(a.rp, b.rp) and np.array_equal(a.ci, b.ci) and sm.same(a.vals, b.vals)


def _check_glue(m, rec, label):
    """the model's reshaping by a second route: a transpose transposed again is its source, a concat split again gives its blocks"""
    op, ids, a = rec
    R = m.t[a["out"]]
    if op == "transpose":
        assert _same_tiling(m._transposed(R), m.t[ids[0]]), f"{label}: transpose twice"
    else:
        pieces = concatref.split(*R.coo(), a["row_sizes"], a["col_sizes"])
        for k, h in enumerate(ids):
            I, J, V = pieces[k // a["grid"][1]][k % a["grid"][1]]
            bi, bj, bv = m.t[h].coo() if h is not None else (np.zeros(0, int), np.zeros(0, int), np.zeros(0, R.dtype))
            assert np.array_equal(I, bi) and np.array_equal(J, bj) and sm.same(V, bv), f"{label}: cell {k} of concat then split"


def walk2(prog, cov, kind):
    """run the model over one program of the second set, collecting the coverage figures"""
    m = sm.Model()
    fresh = {}                           # tiling -> links refreshed source first, one by one, since the chain's base was written
    seen = set()
    for i, rec in enumerate(prog):
        op, ids, a = rec
        dtype = sg.record_dtype(m, rec)
        for h in ids:
            assert h is None or h in m.t or h in m.p, f"step {i}: {rec} names a handle that is not alive"
        built = {h: set(m.t[h].built) for h in ids if h in m.t}
        refresh = op[16:] if op.startswith("set_values_from_") and op[16:] in sm.KINDS2 + ("build",) else None
        if op in ("mxv", "reduce", "spmm"):
            col = a["transpose"] if op != "reduce" else a["dim"] == "cols"
            reads = [(ids[0], "col" if col else "row")]
        elif op in ("step3", "spgemm"):
            p = m.p[ids[0]]
            reads = [(next(h for h, T in m.t.items() if T is x), r) for x, r in ((p.A, "plan_a"), (p.B, "plan_b")) if any(T is x for T in m.t.values())]
        elif op in ("mxv_frontier", "mxv_arg", "reduce_arg"):
            col = a["transpose"] if op != "reduce_arg" else a["dim"] == "cols"
            reads = [(ids[0], ("frontier_" if op == "mxv_frontier" else "arg_") + ("col" if col else "row"))]
        elif op in ("sampled_mxm", "set_values_sampled_mxm"):
            reads = [(ids[1], "sampled_operand"), (ids[2], "sampled_operand")]
        elif op == "trsv":
            reads = [(ids[0], "trsv_" + a["uplo"])]
        elif op == "lu_solve":
            reads = [(ids[0], "trsv_lower"), (ids[0], "trsv_upper")]
        else:
            reads = []
        reads = [(h, m.t[h].last_writer, r) for h, r in reads]
        source_writers = [m.t[s].last_writer for s in ids[1:] if s in m.t] if refresh else []
        trail = m.t[ids[0]].trail if op == "close" else None
        res = m.apply(rec)
        assert (res.status != 0) == ("expect" in a), f"step {i}: {rec}: model status {res.status}"
        cov["steps"] += 1
        if res.status != 0:
            assert res.status == sm.PEM_E_INVALID or a["expect"] in sg.REFUSALS
            cov["refusals"][a["expect"]] += 1
            continue
        cov["ops"][(op, dtype)] += 1
        if op in ("transpose", "concat"):
            _check_glue(m, rec, f"step {i}: {rec}")
        for h, w, r in reads:
            if w is not None:
                cov["pairs"][(w, r)] += 1
            if fresh.get(h, 0) >= 3:
                seen.add("chain")
        for h, before in built.items():
            if h in m.t:
                for s in m.t[h].built - before:
                    cov["first"][s].add(op)
        if op == "ilu0":
            cov["first"]["trsv_lower"].add(op)
        if refresh:
            r = cov["refresh"][refresh]
            r["times"] += 1
            r["after a refresh of another kind"] += any(w is not None and w.startswith("from_") and w != "from_" + refresh for w in source_writers)
            r["after set_values"] += any(w in ("set_values_row", "set_values_col") for w in source_writers)
            r["holding another structure"] += bool(built[ids[0]] - {"map_" + refresh})
        if op.startswith("set_values"):                  # the chain condition: what was refreshed in source-first order
            tid = ids[0]
            srcs = [s for s in sm.sources(m.t[tid].prov) if s in fresh] if "_from_" in op and op[16:] not in ("cplan", "build") else None
            if srcs is None:
                fresh[tid] = 0
            elif srcs:
                fresh[tid] = 1 + max(fresh[s] for s in srcs)
            else:
                fresh.pop(tid, None)
            for j in _downstream(m, tid):
                fresh.pop(j, None)
        trails = [trail] if trail is not None else [T.trail for T in m.t.values()] if i + 1 == len(prog) else []
        for t in trails:
            if _has_subsequence(t, LIFE):
                seen.add("life")
            if "refresh" in t and "source" not in t[:t.index("refresh")] and _has_subsequence(t, CONCAT_LIFE):
                seen.add("concat")
        if op == "close":
            fresh.pop(ids[0], None)
    for s in seen:
        cov[s][kind] += 1


def coverage2():
    cov = dict(steps=0, ops=collections.Counter(), pairs=collections.Counter(), refusals=collections.Counter(),
               first=collections.defaultdict(set), refresh=collections.defaultdict(collections.Counter), chain=collections.Counter(),
               life=collections.Counter(), concat=collections.Counter())
    for seed in sg.SEEDS2:
        walk2(sg.program(seed, sg.STEPS), cov, sg.context_kind(seed))
    return cov


REFRESH_CONDITIONS = ("times", "after a refresh of another kind", "after set_values", "holding another structure")


def table2(cov):
    lines = [f"sequence test coverage, second set: {len(sg.SEEDS2)} seeds x {sg.STEPS} steps = {cov['steps']} steps, "
             f"{sum(cov['refusals'].values())} deliberate refusals"]
    lines.append("operation kind            f64   f32")
    for k in sg.KINDS2_T + sg.KINDS_T + sg.KINDS_P:
        lines.append(f"  {k:24s}{cov['ops'][(k, 'f64')]:5d} {cov['ops'][(k, 'f32')]:5d}")
    lines += [f"  {k:24s}{cov['ops'][(k, None)]:5d}" for k in sg.KINDS_CTX]
    lines.append("writer -> reader          " + " ".join(f"{r:>10s}" for r in READERS + READERS2))
    for w in WRITERS + WRITERS2:
        lines.append(f"  {w:24s}" + " ".join(f"{cov['pairs'][(w, r)]:10d}" for r in READERS + READERS2))
    lines.append("refreshes                 " + "; ".join(REFRESH_CONDITIONS))
    lines += [f"  {k:24s}" + " ".join(f"{cov['refresh'][k][c]:5d}" for c in REFRESH_CONDITIONS) for k in sm.KINDS2 + ("build",)]
    lines.append("first built by")
    lines += [f"  {s:24s}{', '.join(sorted(cov['first'][s]))}" for s in SCHEDULES + MAPS2]
    lines.append("refusals                  " + ", ".join(f"{k} {cov['refusals'][k]}" for k in sg.REFUSALS2 + sg.REFUSALS))
    for what, name in (("chain", "chain of depth 3 refreshed link by link, then read"), ("life", "factor life"), ("concat", "concat between refreshes")):
        lines.append(f"{name}: " + ", ".join(f"{k}: {cov[what][k]} programs" for k in sg.CONTEXT_KINDS))
    return "\n".join(lines)


def test_second_set_seeds_and_text():
    assert len(sg.SEEDS2) == 24 and len(set(sg.SEEDS2) | set(sg.SEEDS)) == 48 and all(sg.op_set(s) == 2 for s in sg.SEEDS2)
    assert all(sg.op_set(s) == 1 for s in sg.SEEDS)
    assert [sg.context_kind(s) for s in sg.SEEDS2[:3]] == list(sg.CONTEXT_KINDS)
    for seed in (sg.SEEDS2[0], sg.SEEDS2[11]):
        a = sg.program(seed, 60)
        assert a == sg.program(seed, 60) and sg.loads(sg.dumps(a)) == a and sg.program(seed, 30) == a[:30]


def test_second_set_coverage_conditions():
    """the model runs every program of SEEDS2, every record is well-typed and none is skipped (walk2 asserts both), and the
    conditions the seed list must meet hold"""
    cov = coverage2()
    print("\n" + table2(cov))
    assert cov["steps"] == len(sg.SEEDS2) * sg.STEPS
    assert sum(cov["ops"].values()) + sum(cov["refusals"].values()) == cov["steps"]
    for k in sg.KINDS2_T:
        for d in ("f64", "f32"):
            assert cov["ops"][(k, d)] >= 10, f"{k} in {d}: {cov['ops'][(k, d)]} times"
    for k in sm.KINDS2:
        r = cov["refresh"][k]
        assert r["times"] >= 4, f"{k}: refreshed {r['times']} times"
        for c in REFRESH_CONDITIONS[1:]:
            assert r[c] >= 1, f"{k}: never refreshed {c}"
    r = cov["refresh"]["build"]              # (a build has no source tiling: the two conditions on its source's writer do not apply)
    assert r["times"] >= 4 and r["holding another structure"] >= 1, f"build: {dict(r)}"
    for k in sg.CONTEXT_KINDS:
        assert cov["chain"][k] >= 1, f"no chain on {k}"
        assert cov["life"][k] >= 1, f"no factor life on {k}"
    assert sum(cov["concat"].values()) >= 1
    for w in WRITERS2:
        for r in READERS:
            assert cov["pairs"][(w, r)] >= 1, f"{w} -> {r}"
    for r in READERS2:
        assert len([w for w in WRITERS + WRITERS2 if cov["pairs"][(w, r)]]) >= 3, f"{r} reads after too few writer kinds"
    for s in SCHEDULES:
        assert len(cov["first"][s]) >= 2, f"{s}: first built only by {sorted(cov['first'][s])}"
    assert sum(cov["refusals"].values()) * 10 <= cov["steps"]
    for k in sg.REFUSALS2:
        assert cov["refusals"][k] >= 3, f"refusal {k}: {cov['refusals'][k]} times"


# ---- the third operation set (sg.SEEDS3) ----------------------------------------------------------------------------------------
SOLVER_LIFE = ("create_lu", "solve", "write", "refresh_factor", "solve", "graph", "solve")
HIERARCHY_LIFE = ("create", "create_amg", "solve", "write", "refresh", "solve", "ctx", "apply", "refresh", "info")
# who built the column schedule of a graph routine's input: no earlier step, an earlier column-orientation reader (a transposed mxv,
# spmm, frontier or arg call, a reduce over the columns, a top-k by column: all build pem_tiled_mxv's schedule), a graph routine
SCHEDULE_STATES = ("none", "reader", "graph")
SCHEDULE_READERS =("mxv", "reduce", "spmm", "mxv_frontier", "mxv_arg", "reduce_arg", "select_topk")


def walk3(prog, cov, kind):
    """run the model over one program of the third set, collecting the coverage figures"""
    m = sm.Model()
    sched_by = {}                        # tiling -> who built its column schedule
    last_graph = None                    # (kind, demand) of the last graph call
    after_trim = False
    ktrail, htrail = {}, {}              # solver / hierarchy -> its events
    since = {}                           # solver -> the events since its last solve
    coloured, ordered, reordered, factored, informed = set(), set(), set(), {}, set()
    done = set()
    for i, rec in enumerate(prog):
        op, ids, a = rec
        dtype = sg.record_dtype(m, rec)
        for h in ids:
            assert h is None or h in m.t or h in m.p or h in m.k or h in m.h, f"step {i}: {rec} names a handle that is not alive"
        built = {h: "mx_cols" in T.built for h, T in m.t.items()}
        res = m.apply(rec)
        assert (res.status != 0) == ("expect" in a), f"step {i}: {rec}: model status {res.status}"
        cov["steps"] += 1
        if res.status != 0:
            cov["refusals"][a["expect"]] += 1
            continue
        cov["ops"][(op, dtype)] += 1
        cov["on"][op].add(kind)
        for h, T in m.t.items():
            if "mx_cols" in T.built and not built.get(h, False):
                sched_by[h] = "graph" if op in sm.GRAPH_KINDS else "reader" if op in SCHEDULE_READERS else "other"
        if op in sm.GRAPH_KINDS:
            T = m.t[ids[0]]
            if not a["symmetric"]:
                cov["state"][(op, sched_by.get(ids[0], "none") if built[ids[0]] else "none")] += 1
            cov["prov"][op].add((T.prov or ("plain",))[0])
            demand = sm.graph_demand(op, T.rows)
            if after_trim:
                cov["after_trim"][op] += 1
            elif last_graph is not None:
                cov["pairs"][(last_graph[0], op)] += 1
                cov["larger"][op] += last_graph[1] > demand
                cov["smaller"][op] += last_graph[1] < demand
            last_graph, after_trim = (op, demand), False
            for k, K in m.k.items():
                if K.a != ids[0]:
                    ktrail[k].append("graph")
        if op == "trim":
            after_trim = True
        if op in ("trim", "reserve"):
            for k in m.k:
                since[k].add(op)
            for h in m.h:
                htrail[h].append("ctx")
        if op.startswith("set_values") and res.wrote in m.t:            # an in-place writer
            w = m.t[res.wrote].last_writer
            for k, K in m.k.items():
                if K.a == res.wrote:
                    ktrail[k].append("write")
                    since[k].add("write:" + w)
                if K.pre == res.wrote and op == "set_values_from_ilu0":
                    ktrail[k].append("refresh_factor")
                    since[k].add("refresh_factor")
            for h, H in m.h.items():
                if H.a == res.wrote:
                    htrail[h] += ["write", "write:" + w]
        if op == "krylov_create":
            K = m.k[a["out"]]
            ktrail[a["out"]], since[a["out"]] = ["create_" + K.precond], set()
            cov["shared"] += sum(1 for J in m.k.values() if J.a == K.a) >= 2
            if K.precond == "amg":
                htrail[K.pre].append("create_amg")
        if op in ("krylov_solve", "tiled_solve"):
            e = res.extra
            status = (e["trail"] if op == "tiled_solve" else m.k[ids[0]].trail)[-1]
            cov["solves"][(e["method"], e["precond"])] += 1
            cov["status"][(e["method"], status)] += 1
            cov["check_every"]["above" if e["check_every"] > e["max_iters"] else e["check_every"]] += 1
        if op == "krylov_solve":
            k, K = ids[0], m.k[ids[0]]
            ktrail[k].append("solve")
            for ev in since[k]:
                cov["solve_after"][ev.split(":")[0]] += 1
                if ev.startswith("write:"):
                    cov["solve_writers"].add(ev[6:])
            since[k] = {ev for ev in since[k] if ev in ("trim", "reserve")}      # (those count since create)
            if K.precond == "amg":
                htrail[K.pre].append("solve")
                cov["solve_after"]["amg_refresh"] += "refresh" in _since_last(htrail[K.pre][:-1], "solve")
            if _has_subsequence(ktrail[k], SOLVER_LIFE) and (m.t[K.pre].prov or ("",))[0] == "ilu0":
                done.add("solver")
            if K.a in reordered and any(F in informed for F, R in factored.items() if R == K.a):
                done.add("reorder")
        if op == "amg_create":
            H = m.h[a["out"]]
            htrail[a["out"]] = ["create"]
            cov["smooth"][a["smooth"]] += 1
            cov["levels"][min(len(H.levels), 3)] += 1
            cov["stalled"] += H.stalled
        if op == "amg_refresh":
            t = htrail[ids[0]]
            cov["refresh_writers"].update(ev[6:] for ev in _since_last(t, "refresh") if ev.startswith("write:"))
            cov["second_refresh"] += "refresh" in t
            cov["refresh_on"][kind] += 1
            t.append("refresh")
        if op == "amg_apply":
            cov["apply_after_refresh"] += "refresh" in htrail[ids[0]]
            htrail[ids[0]].append("apply")
        if op == "amg_info":
            htrail[ids[0]].append("info")
            if _has_subsequence([ev for ev in htrail[ids[0]] if ":" not in ev], HIERARCHY_LIFE) and m.h[ids[0]].opts["refreshable"]:
                done.add("hierarchy")
        if op == "amg_level":
            cov["level_reads"][(a["which"], a["reader"][0])] += 1
            if a["reader"][0] in sm.GRAPH_KINDS:         # (a graph call on the context all the same: the next one follows it)
                last_graph, after_trim = (a["reader"][0], sm.graph_demand(a["reader"][0], m.level_tiling(m.h[ids[0]], a["level"], "A").rows)), False
        if op == "amg_create" and len(m.h[a["out"]].levels) + m.h[a["out"]].stalled > 1:   # (its last aggregate call, likewise)
            L = m.h[a["out"]].levels
            last_graph, after_trim = ("aggregate", sm.graph_demand("aggregate", L[-1 if m.h[a["out"]].stalled else -2]["A"][0])), False
        # the reorder: colour, colour_order, extract with the permutation as both lists, ilu0, trsv_info, a solve
        if op == "colour":
            coloured.add(ids[0])
        if op == "colour_order" and ids[0] in coloured and a["of"] == "colour":
            ordered.add(ids[0])
        if op == "extract" and ids[0] in ordered and a["rows"] == a["cols"] and a["rows"] is not None and a["rows"][0] == "device" \
                and sorted(a["rows"][1]) == list(range(m.t[ids[0]].rows)):
            reordered.add(a["out"])
        if op == "ilu0" and ids[0] in reordered:
            factored[a["out"]] = ids[0]
        if op == "trsv_info" and ids[0] in factored:
            informed.add(ids[0])
    for s in done:
        cov["scenario"][(s, kind)] += 1


def _since_last(trail, what):
    """the events of a trail after the last `what`"""
    k = max((j for j, ev in enumerate(trail) if ev == what), default=-1)
    return trail[k + 1:]


def coverage3():
    C = collections.Counter
    cov = dict(steps=0, ops=C(), refusals=C(), on=collections.defaultdict(set), state=C(), prov=collections.defaultdict(set), pairs=C(),
               larger=C(), smaller=C(), after_trim=C(), solves=C(), status=C(), check_every=C(), solve_after=C(), solve_writers=set(),
               shared=0, smooth=C(), levels=C(), stalled=0, refresh_writers=set(), second_refresh=0, refresh_on=C(),
               apply_after_refresh=0, level_reads=C(), scenario=C())
    for seed in sg.SEEDS3:
        walk3(_program(seed), cov, sg.context_kind(seed))
    return cov


def table3(cov):
    lines = [f"sequence test coverage, third set: {len(sg.SEEDS3)} seeds x {sg.STEPS} steps = {cov['steps']} steps, "
             f"{sum(cov['refusals'].values())} deliberate refusals"]
    lines.append("operation kind            f64   f32  context kinds")
    for k in sg.KINDS3_T:
        lines.append(f"  {k:24s}{cov['ops'][(k, 'f64')]:5d} {cov['ops'][(k, 'f32')]:5d}  {len(cov['on'][k])}")
    lines.append("graph routine             " + " ".join(f"{s:>7s}" for s in SCHEDULE_STATES) + "  larger smaller after_trim  provenances")
    for k in sm.GRAPH_KINDS:
        lines.append(f"  {k:24s}" + " ".join(f"{cov['state'][(k, s)]:7d}" for s in SCHEDULE_STATES) +
                     f"  {cov['larger'][k]:6d} {cov['smaller'][k]:7d} {cov['after_trim'][k]:10d}  {', '.join(sorted(cov['prov'][k]))}")
    lines.append("consecutive graph calls   " + ", ".join(f"{a}->{b} {cov['pairs'][(a, b)]}" for a in sm.GRAPH_KINDS for b in sm.GRAPH_KINDS if a != b))
    lines.append("solves                    " + ", ".join(f"{m} {p} {cov['solves'][(m, p)]}" for m, p in sg.METHOD_PRECOND))
    lines.append("statuses                  " + ", ".join(f"{m} {s} {cov['status'][(m, s)]}" for m in ("cg", "bicgstab") for s in sm.krylovref.STATUS))
    lines.append("a solve after             " + ", ".join(f"{k} {v}" for k, v in sorted(cov["solve_after"].items())) +
                 f"; writers on A {sorted(cov['solve_writers'])}; two solvers on one A {cov['shared']}; check_every {dict(cov['check_every'])}")
    lines.append(f"hierarchies               smooth {dict(cov['smooth'])}, levels (3: three or more) {dict(cov['levels'])}, stalled {cov['stalled']}, "
                 f"second refresh {cov['second_refresh']}, refreshes by context {dict(cov['refresh_on'])}, apply after refresh "
                 f"{cov['apply_after_refresh']}, refresh after writers {sorted(cov['refresh_writers'])}")
    lines.append("level reads               " + ", ".join(f"{w} {r} {n}" for (w, r), n in sorted(cov["level_reads"].items())))
    lines.append("refusals                  " + ", ".join(f"{k} {cov['refusals'][k]}" for k in sg.REFUSALS3))
    for s in sg.SCRIPTS3_ORDER:
        lines.append(f"scenario {s}: " + ", ".join(f"{k}: {cov['scenario'][(s, k)]} programs" for k in sg.CONTEXT_KINDS))
    return "\n".join(lines)


def test_third_set_seeds_and_text():
    assert len(sg.SEEDS3) == 24 and len(set(sg.SEEDS3) | set(sg.SEEDS2) | set(sg.SEEDS)) == 72 and all(sg.op_set(s) == 3 for s in sg.SEEDS3)
    assert all(sg.op_set(s) == 2 for s in sg.SEEDS2) and all(sg.op_set(s) == 1 for s in sg.SEEDS)
    assert [sg.context_kind(s) for s in sg.SEEDS3[:3]] == list(sg.CONTEXT_KINDS)
    for seed in (sg.SEEDS3[0], sg.SEEDS3[11]):
        a = sg.program(seed, 60)
        assert a == sg.program(seed, 60) and sg.loads(sg.dumps(a)) == a and sg.program(seed, 30) == a[:30]


def test_third_set_coverage_conditions():
    """the model runs every program of SEEDS3, every record is well-typed and none is skipped (walk3 asserts both), and the
    conditions the seed list must meet hold"""
    cov = coverage3()
    print("\n" + table3(cov))
    assert cov["steps"] == len(sg.SEEDS3) * sg.STEPS
    assert sum(cov["ops"].values()) + sum(cov["refusals"].values()) == cov["steps"]
    for k in sg.KINDS3_T:
        for d in ("f64", "f32"):
            assert cov["ops"][(k, d)] >= 10, f"{k} in {d}: {cov['ops'][(k, d)]} times"
        assert cov["on"][k] == set(sg.CONTEXT_KINDS), f"{k} runs on {sorted(cov['on'][k])} only"
    for k in sg.REFUSALS3:
        assert cov["refusals"][k] >= 1, f"refusal {k} is never emitted"
    assert sum(cov["refusals"].values()) * 10 <= cov["steps"]
    # the graph routines: the state of the column schedule, the provenance of the input, the order of the calls
    for k in sm.GRAPH_KINDS:
        for s in SCHEDULE_STATES:
            assert cov["state"][(k, s)] >= 1, f"{k} never runs on a tiling whose column schedule is '{s}'"
        assert len(cov["prov"][k]) >= 3, f"{k} runs on the provenances {sorted(cov['prov'][k])} only"
        assert cov["larger"][k] >= 1 and cov["smaller"][k] >= 1, f"{k}: after a larger demand {cov['larger'][k]}, a smaller {cov['smaller'][k]}"
        assert cov["after_trim"][k] >= 1, f"{k} is never the first graph call after a trim"
        for j in sm.GRAPH_KINDS:
            assert j == k or cov["pairs"][(j, k)] >= 1, f"{k} never follows {j}"
    seen = set().union(*cov["prov"].values())
    assert set(sm.KINDS2) | {"cplan"} <= seen, f"no graph routine runs on a tiling made by {sorted((set(sm.KINDS2) | {'cplan'}) - seen)}"
    # solves
    for m, p in sg.METHOD_PRECOND:
        assert cov["solves"][(m, p)] >= 3, f"{m} with {p}: {cov['solves'][(m, p)]} solves"
    for m in ("cg", "bicgstab"):
        for s in sm.krylovref.STATUS:
            assert cov["status"][(m, s)] >= 1, f"{m} never ends as {s}"
    assert len(cov["solve_writers"]) >= 3, f"a solve follows the writers {sorted(cov['solve_writers'])} on A only"
    for ev in ("refresh_factor", "amg_refresh", "trim", "reserve"):
        assert cov["solve_after"][ev] >= 1, f"no solve after {ev}"
    assert cov["shared"] >= 1 and cov["check_every"]["above"] >= 1 and cov["check_every"][1] >= 1
    # hierarchies
    assert cov["smooth"][0] >= 1 and cov["smooth"][1] >= 1
    for n in (1, 2, 3):
        assert cov["levels"][n] >= 1, f"no hierarchy of {n} levels{' or more' if n == 3 else ''}"
    assert cov["stalled"] >= 1 and len(cov["refresh_writers"]) >= 3 and cov["second_refresh"] >= 1 and cov["apply_after_refresh"] >= 1
    assert cov["refresh_on"]["graph_replay"] >= 4
    for w in "APR":
        assert any(cov["level_reads"][(w, r)] for r in ("mxv", "reduce", "export_csr")), f"{w}_l is never read"
    assert any(cov["level_reads"][("A", r)] for r in ("colour", "components", "mis", "aggregate")), "no graph routine runs on a borrowed A_l"
    # the three scenarios run to their end
    for s in sg.SCRIPTS3_ORDER:
        for k in sg.CONTEXT_KINDS:
            assert cov["scenario"][(s, k)] >= 2, f"scenario {s} on {k}: {cov['scenario'][(s, k)]} programs"


@pytest.mark.parametrize("mutation", sm.MUTATIONS)
def test_negative_controls_are_visible_to_the_runner(mutation):
    """each model mutation changes something the runner observes, at the step tests/test_gpu_seq.py expects"""
    import seqcontrol
    seed, where = seqcontrol.NEGATIVE[mutation]
    assert seqcontrol.first_divergence(_program(seed) if seed in sg.SEEDS else sg.program(seed, sg.STEPS), mutation) == where
