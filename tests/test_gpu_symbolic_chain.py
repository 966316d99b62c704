"""The symbolic phase with its glue folded away: step 1's row bins in one launch on the main stream where a plan
allows it (PEM_OPT_S1_ONE_LAUNCH), its row classification scanning its own row totals (PEM_OPT_S1_CLASS_SCAN) and, on repeat
passes, step 2's offsets kernel summing the group counts in front of its groups itself (PEM_OPT_S2_TAIL_FOLD).  None of them
changes an output word: every plan array against the oracle's, bit for bit, with each option forced on and off, with and
without graph replay, on the first pass, on repeat passes and after spgemm(); spgemm(); step2(); step3() -- at the sizes where
each path begins and ends, and on inputs that must fall back."""
import numpy as np
import pytest

from matgen import _grouped, cases
from prune_ref import expected

pytestmark = pytest.mark.gpu

CASES = cases()
C_NAMES = ["c_tile_rowptr", "c_tile_rowidx", "c_tile_colidx", "pairs_offset", "pairs_a", "pairs_b", "c_mask", "c_tile_nnz_ptr",
           "c_rowptr", "c_rowcolidx", "c_vals"]
RC_THREADS, RC_BLOCKS = 512, 128          # s1_rowclass_kernel<.., SCAN>: rows per workgroup, workgroups of the chained scan
S2_GROUP, S2_FOLD_GROUPS = 256, 8192      # C tiles per group, groups the folded offsets kernel takes


def tile_rows_case(mt, seed=7):
    """A square matrix of exactly mt tile rows (16 * mt - 3 rows) whose tile rows differ widely in live products: random entries,
    one hub row and one hub column; every tile row holds an entry, so no row total of the scan is trivially zero."""
    rng = np.random.default_rng(seed + mt)
    n = 16 * mt - 3 if mt > 1 else 13
    m = min(5 * mt + 40, 400_000)
    I = np.concatenate([rng.integers(0, n, m), np.arange(0, n, 16), np.full(min(n, 3000), n // 2), rng.integers(0, n, min(n, 3000))])
    J = np.concatenate([rng.integers(0, n, m), rng.integers(0, n, len(np.arange(0, n, 16))), rng.choice(n, min(n, 3000), replace=False),
                        np.full(min(n, 3000), n // 3)])
    key = rng.permutation(np.unique(I.astype(np.int64) * n + J))
    V = rng.uniform(-1.0, 1.0, len(key))
    V[V == 0.0] = 0.25
    return n, n, (key // n).astype(np.int32), (key % n).astype(np.int32), V, False


def c_tiles_case(ntc):
    """A square matrix whose square has exactly ntc C tiles of one pair each (a shallow plan) on few tile rows and columns (the
    oracle's plan costs tile rows x tile columns): tiles (i, 0) for i < a with one or two entries in global column 0, tiles (0, j)
    for j < b with an entry in global row 0 -- C tile (i, j) for every i < a, j < b, of one or two entries, so the group counts
    differ and a wrong base shows -- and ntc - a * b isolated diagonal tiles behind them."""
    b = min(ntc, 1024)
    a = ntc // b
    rem = ntc - a * b
    i, j = np.arange(a, dtype=np.int64), np.arange(b, dtype=np.int64)
    two = i[i % 3 >= 1]
    d = 16 * (max(a, b) + np.arange(rem, dtype=np.int64)) + 3
    I = np.concatenate([16 * i + i % 16, 16 * two + (two + 5) % 16, np.zeros(b, np.int64), d])
    J = np.concatenate([np.zeros(a, np.int64), np.zeros(len(two), np.int64), 16 * j + (5 * j) % 16, d])
    n = 16 * (max(a, b) + rem)
    key = np.unique(I * n + J)
    V = 0.5 + (key % 7).astype(np.float64) / 8.0
    return n, n, (key // n).astype(np.int32), (key % n).astype(np.int32), V, False


def bins_case(counts, hubs, rows=400_000, seed=5):
    """A (rows x 16 * len(counts)) for A * A^T (matgen._grouped): a tile row with an entry in group k has about counts[k] live
    products, one with entries in several groups their sum; hubs: (row, groups) with an entry in each of the groups."""
    return _grouped(np.random.default_rng(seed), rows, len(counts), counts, hubs)


def row_products(case):
    """tile-level products per tile row of A * A^T (an upper bound of the live ones; pruning takes a few per cent)"""
    rows, cols, I, J, V, tr = case
    w = cols // 16 + 1
    t = np.unique((I.astype(np.int64) // 16) * w + J // 16)
    ti, tj = t // w, t % w
    return np.bincount(ti, weights=np.bincount(tj)[tj]).astype(np.int64)


_MIXED = [30, 30, 50, 300, 300, 400, 1500, 1800, 3000, 2500, 2000, 40]
BINS = {
    # every role at once: tiny, 512, 2048, 8192 and a handful of rows above 8192 keys (in segments)
    "every_role": (_MIXED, [(1234, [6, 7, 8, 9, 10]), (77777, [7, 8, 9, 10]), (5, [0, 1, 2])]),
    # no tiny and no 512-key rows
    "no_small_rows": ([3000, 2500, 2000, 1500], [(9, [0, 1, 2, 3])]),
    # tiny rows alone
    "tiny_only": ([30, 40, 50, 20], []),
}


_CACHE = {}


def _prepared(pkg, oracle, ctx, key, case):
    """GPU tilings per call, the oracle's arrays once per session (the largest cases take the oracle seconds)."""
    rows, cols, I, J, V, tr = case
    gA = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, False)
    gB = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, True) if tr else gA
    if key not in _CACHE:
        oA = oracle.Tiled(rows, cols, I, J, V, False)
        oB = oracle.Tiled(rows, cols, I, J, V, True) if tr else oA
        _CACHE[key] = expected(oracle.Plan(oA, oB), oA, oB)
    return gA, gB, _CACHE[key]


def _check(plan, want, what):
    want_arrays, want_counts = want
    info = plan.info()
    assert (info["ntiles_c"], info["npairs"], info["nnz_c"], info["npairs_all"]) == want_counts, what
    for arr in C_NAMES:
        got = plan.array(arr)
        assert got.dtype == want_arrays[arr].dtype and np.array_equal(got, want_arrays[arr]), f"{what}: plan array {arr} differs"


def _protocol(pkg, ctx, gA, gB, want, opts, graph, what):
    ctx.set_graph_replay(graph)
    try:
        plan = pkg.CPlan(ctx, gA, gB)
        for k, v in opts.items():
            plan.set_option(k, v)
        plan.spgemm()                                 # first pass: every size read back
        _check(plan, want, what + " / first pass")
        plan.spgemm()                                 # repeat pass (graph replay: the capture)
        _check(plan, want, what + " / repeat pass")   # (reads Ctiles_rowColIdx: on demand, from the group counts the pass left)
        plan.spgemm()                                 # ... and one on top of the arrays materialised on demand
        plan.spgemm()
        _check(plan, want, what + " / third repeat pass")
        plan.step2()                                  # the step-wise API on top of a repeat pass's state
        plan.step3()
        _check(plan, want, what + " / spgemm, spgemm, step2, step3")
        plan.spgemm()
        _check(plan, want, what + " / pass after the step-wise calls")
    finally:
        ctx.set_graph_replay(False)


def _kernels_of_repeat_pass(pkg, ctx, gA, gB, opts, passes_before=1):
    plan = pkg.CPlan(ctx, gA, gB)
    for k, v in opts.items():
        plan.set_option(k, v)
    for _ in range(passes_before):
        plan.spgemm()
    ctx.set_kernel_profiling(True)
    try:
        ctx.reset_kernel_stats()
        plan.spgemm()
        return set(ctx.kernel_stats())
    finally:
        ctx.set_kernel_profiling(False)


MODES = [(cs, tf, g) for cs in (1, 0) for tf in (1, 0) for g in (False, True)]   # (the row bins: as the plan chooses)


@pytest.mark.parametrize("name", ["powerlaw_600", "hub_row_4000", "blockrows_1600", "blockrows_10000", "xl_mixed_AAt", "band_1500", "dense_48",
                                  "one_entry", "empty_matrix", "empty_rows", "rect_70x40_AAt", "hub_tile_2100_AAt"])
def test_matgen_cases_every_mode(pkg, oracle, ctx, name):
    """Inputs that fill every row bin, the oversized rows, deep plans (whose entry kernel keeps the scan) and the empty product."""
    gA, gB, want = _prepared(pkg, oracle, ctx, ("matgen", name), CASES[name])
    for cs, tf, g in MODES:
        _protocol(pkg, ctx, gA, gB, want, {"s1_class_scan": cs, "s2_tail_fold": tf}, g, f"{name} class_scan={cs} tail_fold={tf} graph={g}")


@pytest.mark.parametrize("hook", [{"s1_force_key64": 1}, {"s1_xlcap": 300}, {"s1_segments": 1}, {"s1_serial": 1}, {"s3_decode": 0}])
def test_with_the_other_step1_and_step2_paths(pkg, oracle, ctx, hook):
    """64-bit keys, oversized rows, column-range segments, serial bins, and Ctiles_rowColIdx written on the pass (the entry kernel:
    not folded) under the folded glue."""
    gA, gB, want = _prepared(pkg, oracle, ctx, ("matgen", "hub_row_4000"), CASES["hub_row_4000"])
    for cs, tf, g in MODES:
        _protocol(pkg, ctx, gA, gB, want, dict(hook, s1_class_scan=cs, s2_tail_fold=tf), g, f"{hook} class_scan={cs} tail_fold={tf} graph={g}")


@pytest.mark.parametrize("mt", [1, RC_THREADS - 1, RC_THREADS, RC_THREADS + 1, 3 * RC_THREADS + 17, RC_THREADS * RC_BLOCKS,
                                RC_THREADS * RC_BLOCKS + 1])
def test_row_scan_inside_the_classification(pkg, oracle, ctx, mt):
    """Tile-row counts at one row, around one workgroup's rows, over a few workgroups, at the largest count the chained scan takes
    (128 workgroups) and the first one beyond it, where the classification is followed by the scan launch as before."""
    case = tile_rows_case(mt)
    gA, gB, want = _prepared(pkg, oracle, ctx, ("rows", mt), case)
    assert gA.tile_rows == mt
    names = _kernels_of_repeat_pass(pkg, ctx, gA, gB, {})
    in_range = mt <= RC_THREADS * RC_BLOCKS
    assert ("s1_rowclass_kernel<scan>" in names) == in_range and ("s1_rowclass_kernel" in names) == (not in_range), names
    assert "s1_rowclass_kernel<scan>" not in _kernels_of_repeat_pass(pkg, ctx, gA, gB, {"s1_class_scan": 0})
    for cs in (1, 0):
        for g in (False, True):
            _protocol(pkg, ctx, gA, gB, want, {"s1_class_scan": cs}, g, f"mt={mt} class_scan={cs} graph={g}")


@pytest.mark.parametrize("ntc", [1, S2_GROUP - 1, S2_GROUP, S2_GROUP + 1, 2 * S2_GROUP, 5 * S2_GROUP + 3,
                                 S2_GROUP * S2_FOLD_GROUPS, S2_GROUP * S2_FOLD_GROUPS + 1])
def test_step2_tail_in_one_launch(pkg, oracle, ctx, ntc):
    """Group counts at 1, 2, a few, the bound (8192 groups) and the bound + 1 (the scan launch as before): C_nnz, Ctiles_nnz_ptr,
    and Ctiles_rowColIdx materialised on demand from the counts the folded kernel leaves unscanned."""
    case = c_tiles_case(ntc)
    gA, gB, want = _prepared(pkg, oracle, ctx, ("ctiles", ntc), case)
    assert want[1][0] == ntc
    ngroups = (ntc + S2_GROUP - 1) // S2_GROUP
    names = _kernels_of_repeat_pass(pkg, ctx, gA, gB, {})
    folded = ngroups <= S2_FOLD_GROUPS
    assert ("s2_offsets_kernel<fold>" in names) == folded and ("s2_offsets_kernel" in names) == (not folded), names
    assert "s2_offsets_kernel<fold>" not in _kernels_of_repeat_pass(pkg, ctx, gA, gB, {"s2_tail_fold": 0})
    for tf in (1, 0):
        for g in (False, True):
            _protocol(pkg, ctx, gA, gB, want, {"s2_tail_fold": tf}, g, f"ntc={ntc} tail_fold={tf} graph={g}")


def test_option_change_restarts_a_plan_with_folded_glue(pkg, oracle, ctx):
    """Changing an option that changes the sizes (PEM_OPT_PRUNE) starts the plan over: the first pass after it takes the scan
    launches and reads the sizes back, the repeat passes fold again -- and the repeat pass's size check, which now rides on the
    lane that computes C_nnz, accepts them."""
    gA, gB, want = _prepared(pkg, oracle, ctx, ("matgen", "powerlaw_600"), CASES["powerlaw_600"])
    plan = pkg.CPlan(ctx, gA, gB)
    for _ in range(3):
        plan.spgemm()
    _check(plan, want, "pruned")
    plan.set_option("prune", 0)                       # other sizes: P, T_C stay, the pair count grows
    for _ in range(3):
        plan.spgemm()
    plan.set_option("prune", 1)
    for _ in range(3):
        plan.spgemm()
    _check(plan, want, "pruned again")


@pytest.mark.parametrize("name", list(BINS))
def test_row_bins_in_one_launch(pkg, oracle, ctx, name):
    """PEM_OPT_S1_ONE_LAUNCH: inputs that fill every role of s1_bins_kernel at once, or leave some empty; forced on, chosen by the
    plan (2) and off, with and without graph replay: pair lists, pair_col heads (through _C_tileColIdx / the pair offsets) and
    _C_rowPtr against the oracle's.  The kernel must really run where the plan allows it, and only there."""
    case = bins_case(*BINS[name])
    p = row_products(case)
    pop = [int(((p > lo) & (p <= hi)).sum()) for lo, hi in ((0, 64), (64, 512), (512, 2048), (2048, 8192), (8192, 1 << 18))]
    if name == "every_role":
        assert all(pop) and pop[4] < 8, pop
    gA, gB, want = _prepared(pkg, oracle, ctx, ("bins", name), case)
    for one in (1, 2, 0):
        names = _kernels_of_repeat_pass(pkg, ctx, gA, gB, {"s1_one_launch": one})
        assert ("s1_bins_kernel" in names) == (one != 0), (one, names)
        assert any(k.startswith(("s1_rowsort", "s1_tiny", "s1_rowseg")) for k in names) == (one == 0), (one, names)
        for g in (False, True):
            _protocol(pkg, ctx, gA, gB, want, {"s1_one_launch": one}, g, f"{name} one_launch={one} graph={g}")


def test_one_launch_single_row(pkg, oracle, ctx):
    """a single tile row, a single entry"""
    for nm in ("one_entry", "dense_tile", "tiny_9x9"):
        gA, gB, want = _prepared(pkg, oracle, ctx, ("matgen", nm), CASES[nm])
        for one in (1, 2, 0):
            for g in (False, True):
                _protocol(pkg, ctx, gA, gB, want, {"s1_one_launch": one}, g, f"{nm} one_launch={one} graph={g}")


@pytest.mark.parametrize("hook", [{}, {"s1_force_key64": 1}, {"s1_xlcap": 300}, {"s1_serial": 1}])
@pytest.mark.parametrize("name", ["every_role", "blockrows_10000", "xl_mixed_AAt"])
def test_one_launch_falls_back(pkg, oracle, ctx, name, hook):
    """64-bit keys, oversized rows (PEM_OPT_S1_XLCAP; xl_mixed_AAt has them without a hook) and serial bins keep the forked bins
    also with the option forced on; a plan with more segments than CUs (blockrows_10000: a hundred 10 000-key rows) keeps them
    unless it is forced.  Whatever runs gives the oracle's arrays."""
    case = bins_case(*BINS[name]) if name in BINS else CASES[name]
    gA, gB, want = _prepared(pkg, oracle, ctx, ("bins" if name in BINS else "matgen", name), case)
    for one in (1, 2):
        names = _kernels_of_repeat_pass(pkg, ctx, gA, gB, dict(hook, s1_one_launch=one))
        expect = not hook and (name == "every_role" or (name == "blockrows_10000" and one == 1))
        assert ("s1_bins_kernel" in names) == expect, (one, names)
        for g in (False, True):
            _protocol(pkg, ctx, gA, gB, want, dict(hook, s1_one_launch=one), g, f"{name} {hook} one_launch={one} graph={g}")
