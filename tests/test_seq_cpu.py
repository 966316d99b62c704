"""CPU: what the sequence test (tests/seqgen.py, tests/seqmodel.py, tests/test_gpu_seq.py) can check without a GPU.

  - program(seed, steps) is a pure function of its arguments and its text form round-trips;
  - the model alone executes every committed program, every record is well-typed, none is skipped;
  - the model's plan results agree with oracle.Plan (the tiled restatement: another route than the model's oracle.csr_spgemm /
    semiringref) at every spgemm step: this guards the model's glue, the references have their own CPU tests;
  - the coverage conditions the committed seed list must meet (test_coverage_conditions).  They are conditions, not measurements:
    if a change to the generator misses one, change the weights or add seeds.

One condition is read narrower than it could be: each derivation map (C^T's, ewise's, select's) can only be built by its own
set_values_from_* entry point, so "first built by two different operation kinds" cannot hold for it; asserted instead is that each
is built at least twice and at least once on a tiling that already holds another lazily built structure.
"""
import collections

import numpy as np
import pytest

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
            assert h is None or h in m.t or h in m.p, f"step {i}: {rec} names a handle that is not alive"
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


def coverage(oracle=None):
    cov = dict(steps=0, ops=collections.Counter(), pairs=collections.Counter(), refusals=collections.Counter(),
               first=collections.defaultdict(set), maps=collections.defaultdict(list), scenario=collections.Counter())
    for seed in sg.SEEDS:
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
    cov = coverage(oracle)
    assert cov["steps"] == len(sg.SEEDS) * sg.STEPS
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


@pytest.mark.parametrize("mutation", sm.MUTATIONS)
def test_negative_controls_are_visible_to_the_runner(mutation):
    """each model mutation changes something the runner observes, at the step tests/test_gpu_seq.py expects"""
    import seqcontrol
    seed, where = seqcontrol.NEGATIVE[mutation]
    assert seqcontrol.first_divergence(_program(seed) if seed in sg.SEEDS else sg.program(seed, sg.STEPS), mutation) == where
