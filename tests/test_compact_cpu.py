"""The compaction of tests/compactref.py is exact: where the plain oracle still runs, the oracle's results on the compacted
operands, lifted back, equal its results on the operands themselves array for array (no GPU)."""
import numpy as np
import pytest

import compactref
from compactref import T_NAMES, Product, lift_coo, lift_csr, lift_plan_arrays, row_products
from matgen import BIGDIM_RUNGS, HYPER_N, bigdim_case, cases, hypersparse
from prune_ref import C_NAMES, expected

NAMES = ["k64_bins", "wide_tilecols", "hub_tile_2100_AAt", "empty_rows", "ragged_37"]


@pytest.fixture(scope="module")
def all_cases():
    return cases()


def test_line_map_round_trip_and_pointer_check():
    idx = np.array([5, 17, 16, 400, 415, 1_000_000_004], np.int64)
    m = compactref.compact(idx >> 4, 1_000_000_005)
    assert m.used.tolist() == [0, 1, 25, 62_500_000] and m.cdim == 64 and m.tiles == 62_500_001
    new = m.fwd(idx)
    assert new.tolist() == [5, 17, 16, 32, 47, 52] and np.array_equal(m.inv(new), idx.astype(np.int32))
    assert np.all(np.diff(m.fwd(np.sort(idx))) > 0), "the map is monotone"
    with pytest.raises(AssertionError):
        m.fwd([48])
    small = compactref.compact([1, 3], 70)
    ptr_c = np.array([0, 2, 5], np.int32)
    full = small.expand_ptr(ptr_c)
    assert full.tolist() == [0, 0, 2, 2, 5, 5] and small.ptr_matches(full, ptr_c)
    for bad in ([0, 0, 2, 2, 5, 4], [0, 1, 2, 2, 5, 5], [0, 0, 2, 3, 5, 5], [0, 0, 2, 2, 5, 6], [1, 0, 2, 2, 5, 5]):
        assert not small.ptr_matches(np.array(bad, np.int32), ptr_c), bad
    assert not small.ptr_matches(full.astype(np.int64), ptr_c) and not small.ptr_matches(full[:-1], ptr_c)
    assert small.expand_line_ptr(np.arange(33, dtype=np.int32)).tolist() == [0] * 17 + list(range(1, 17)) + [16] * 16 + list(range(17, 33)) + [32] * 6


@pytest.mark.parametrize("name", NAMES)
def test_lifted_compacted_oracle_equals_plain_oracle(oracle, all_cases, name):
    case = all_cases[name]
    rows, cols, I, J, V, tr = case
    c = Product(oracle, case)
    oA = oracle.Tiled(rows, cols, I, J, V, False)
    oB = oracle.Tiled(rows, cols, I, J, V, True) if tr else oA
    for lifted, o in ((c.A, oA), (c.B, oB)):
        assert (lifted.rows, lifted.cols, lifted.nnz, lifted.tile_rows, lifted.tile_cols, lifted.ntiles) == \
            (o.rows, o.cols, o.nnz, o.tile_rows, o.tile_cols, o.ntiles)
        for arr in T_NAMES:
            got, want = lifted.array(arr), getattr(o, arr)
            assert got.dtype == want.dtype and np.array_equal(got, want), f"{name}: tiled array {arr}"
            assert lifted.matches(arr, want), f"{name}: matches({arr})"
    op = oracle.Plan(oA, oB)
    assert oracle.flop_count(c.oA, c.oB) == oracle.flop_count(oA, oB)
    for prune in (False, True):
        want, want_counts = expected(op, oA, oB, prune)
        got_c, got_counts = expected(c.op, c.oA, c.oB, prune)
        assert got_counts == want_counts
        got = lift_plan_arrays(got_c, c.rmap, c.cmap)
        for arr in C_NAMES:
            assert got[arr].dtype == want[arr].dtype and np.array_equal(got[arr], want[arr]), f"{name}: plan array {arr} (prune={prune})"
        assert c.rmap.ptr_matches(want["c_tile_rowptr"], got_c["c_tile_rowptr"])
        if len(c.rmap.used):
            full = np.zeros(c.rmap.tiles, np.int64)
            full[c.rmap.used] = row_products(got_c)
            assert np.array_equal(full, row_products(want))
    for a, b in zip(lift_coo(*c.op.export_coo(), c.rmap, c.cmap), op.export_coo()):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    for a, b in zip(lift_csr(*c.op.export_csr(), c.rmap, c.cmap), op.export_csr()):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    for f32 in (False, True):
        Vr = V.astype(np.float32).astype(np.float64) if f32 else V
        sa, sb = oracle.Csr(rows, cols, I, J, Vr, False), oracle.Csr(rows, cols, I, J, Vr, tr)
        rp, ci, v = oracle.csr_spgemm(sa, sb, 1, f32=f32).arrays()
        (r1, c1, v1), compacted = c.csr_spgemm_coo(f32=f32, values=Vr)
        assert np.array_equal(r1, np.repeat(np.arange(rows, dtype=np.int32), np.diff(rp))) and np.array_equal(c1, ci)
        assert np.array_equal(v1, v), "the ascending-k chain is unchanged: values bit for bit"
        for a, b in zip(lift_csr(*compacted, c.rmap, c.cmap), (rp, ci, v)):
            assert a.dtype == b.dtype and np.array_equal(a, b)


def bins_of(nl):
    """populations of step 1's row lists by live products per tile row, for B with more than 2^17 tile columns (no 32768-key bin)"""
    edges = [(1, 64), (65, 512), (513, 2048), (2049, 8192), (8193, 1 << 62)]
    return [int(((nl >= lo) & (nl <= hi)).sum()) for lo, hi in edges]


@pytest.mark.parametrize("rung", [20, 22, 24])
def test_bigdim_cases_reach_every_row_list(oracle, rung):
    """the ladder's cases: B's tile columns cross the rung's power of two, the last row holds an entry, and every row list of step 1
    is populated with pruning on and off -- the tiny bin, the 512, 2048 and 8192 bins and at least two oversized rows"""
    case = bigdim_case(rung)
    rows, cols, I, J, V, tr = case
    T = BIGDIM_RUNGS[rung]
    assert tr and rows == 16 * T + 5 and cols == 640 and (rows + 15) // 16 == T + 1 and 1 << (rung - 1) < T + 1 <= 1 << rung
    assert rows < 2 ** 31 and int(I.max()) == rows - 1
    c = Product(oracle, case)
    for prune in (True, False):
        arrays, _ = expected(c.op, c.oA, c.oB, prune)
        pop = bins_of(row_products(arrays))
        assert min(pop[:4]) >= 1 and pop[4] >= 2, (rung, prune, pop)


def test_hypersparse_is_past_the_chained_scan_everywhere(oracle):
    n, I, J, V, S = hypersparse()
    lim = 262_144
    assert n == HYPER_N and (n + 15) // 16 > lim and len(S) == 400
    assert {0, 15, 16, 4_194_303, 4_194_304, 4_194_319, 4_194_320, n - 1} <= set(S.tolist())
    key = I.astype(np.int64) * n + J
    assert len(np.unique(key)) == len(key) > lim
    assert len(np.unique((I.astype(np.int64) >> 4) * (1 << 20) + (J >> 4))) > lim
    assert ((I >> 4 == lim) & (J >> 4 == lim)).sum() == 256, "one dense tile in tile row 262 144"
    c = Product(oracle, (n, n, I, J, V, False), plan=False)
    (r, cc, v), _ = c.csr_spgemm_coo()
    assert len(r) > lim and len(np.unique((r.astype(np.int64) >> 4) * (1 << 20) + (cc >> 4))) > lim
    assert int(r.max()) == n - 1 or int(cc.max()) == n - 1


def test_product_coo_and_lifted_tiled_equal_the_plain_oracle(oracle, all_cases):
    rows, cols, I, J, V, _ = all_cases["empty_rows"]
    rng = np.random.default_rng(5)
    k = rng.choice(rows * cols, 700, replace=False)
    b = ((k // cols).astype(np.int32), (k % cols).astype(np.int32), rng.uniform(-1, 1, len(k)))
    rp, ci, v = oracle.csr_spgemm(oracle.Csr(rows, cols, I, J, V), oracle.Csr(rows, cols, *b)).arrays()
    r1, c1, v1 = compactref.product_coo(oracle, rows, (I, J, V), b)
    assert np.array_equal(r1, np.repeat(np.arange(rows, dtype=np.int32), np.diff(rp))) and np.array_equal(c1, ci) and np.array_equal(v1, v)
    rows, cols, I, J, V, _ = all_cases["wide_tilecols"]
    for tr in (False, True):
        o, lifted = oracle.Tiled(rows, cols, I, J, V, tr), compactref.lifted_tiled(oracle, rows, cols, I, J, V, tr)
        assert (lifted.rows, lifted.cols, lifted.tile_rows, lifted.tile_cols, lifted.ntiles) == (o.rows, o.cols, o.tile_rows, o.tile_cols, o.ntiles)
        for arr in T_NAMES:
            assert lifted.matches(arr, getattr(o, arr)) and np.array_equal(lifted.array(arr), getattr(o, arr)), (tr, arr)


def test_index_map_vector_references_equal_the_full_ones(oracle, all_cases):
    """mxvref / frontierref on the used lines only, scattered back, equal the references on the whole matrix"""
    import frontierref as fr
    import mxvref as mr
    rows, cols, I, J, V, _ = all_cases["empty_rows"]
    m = compactref.IndexMap(np.concatenate([I, J]), rows)
    assert m.cdim < rows
    o = np.lexsort((J, I))
    rp = np.zeros(rows + 1, np.int64)
    np.cumsum(np.bincount(I, minlength=rows), out=rp[1:])
    full, comp = (rp, J[o].astype(np.int64), V[o]), m.csr(I, J, V)
    rng = np.random.default_rng(9)
    x, y0 = rng.standard_normal(rows), rng.standard_normal(rows)
    present = rng.random(rows) < 0.3
    for tr in (False, True):
        for s in mr.SEMIRINGS:
            for acc in (None, y0):
                want = mr.mxv(rows, cols, *full, x, s, np.float64, y0=acc, oracle=oracle, transpose=tr)
                got = mr.mxv(m.cdim, m.cdim, *comp, m.gather(x), s, np.float64, y0=None if acc is None else m.gather(acc), oracle=oracle,
                             transpose=tr)
                assert np.array_equal(m.scatter(got, mr.MXV_START[s] if acc is None else acc), want, equal_nan=True), (tr, s)
        for op in mr.OPS:
            dim = "cols" if tr else "rows"
            want = mr.reduce(rows, cols, *full, op, np.float64, dim=dim)
            assert np.array_equal(m.scatter(mr.reduce(m.cdim, m.cdim, *comp, op, np.float64, dim=dim), mr.IDENTITY[op]), want)
        wy, wp = fr.mxv_frontier(rows, cols, *full, x, "min_plus", np.float64, present=present, transpose=tr)
        gy, gp = fr.mxv_frontier(m.cdim, m.cdim, *comp, m.gather(x), "min_plus", np.float64, present=m.gather(present), transpose=tr)
        assert np.array_equal(m.scatter(gy, np.inf), wy) and np.array_equal(m.scatter(gp, 0), wp)


# ---- the lifting rules of the graph routines, the solves and the arg folds (compactref, second half) --------------------------------
def _isolated_610():
    """700 vertices of which 610 carry no off-diagonal entry (20 of those a diagonal entry only); the pattern is not symmetric"""
    rng = np.random.default_rng(17)
    n = 700
    act = np.sort(rng.choice(n, 90, replace=False))
    k = rng.choice(90 * 90, 400, replace=False)
    I, J = act[k // 90], act[k % 90]
    used = np.unique(np.concatenate([I[I != J], J[I != J]]))
    assert len(used) == 90
    lone = rng.choice(np.setdiff1d(np.arange(n), act), 20, replace=False)
    I, J = np.concatenate([I, lone]), np.concatenate([J, lone])
    p = rng.permutation(len(I))
    return n, I[p].astype(np.int32), J[p].astype(np.int32), rng.uniform(-1.0, 1.0, len(I))


@pytest.fixture(scope="module")
def lift_graphs(all_cases):
    out = {name: (all_cases[name][0], *all_cases[name][2:5]) for name in ("empty_rows", "ragged_37")}
    out["isolated_610"] = _isolated_610()
    return out


LIFT_NAMES = ["isolated_610", "empty_rows", "ragged_37"]


def _with_diagonal(n, I, J, V):
    """the recipe of matgen.hypersparse_diag on a small matrix"""
    off = I != J
    I, J, V = I[off], J[off], V[off]
    d = 4.0 + np.bincount(I, weights=np.abs(V), minlength=n)
    k = np.arange(n, dtype=np.int32)
    return np.concatenate([I, k]), np.concatenate([J, k]), np.concatenate([V, d]), d


def _full_csr(n, I, J, V):
    o = np.lexsort((J, I))
    rp = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(I, minlength=n), out=rp[1:])
    return rp, J[o].astype(np.int64), np.asarray(V)[o]


def test_hash_priority_at_is_the_hash():
    import colourref as cr
    for seed in (0, 5, 12345, 2 ** 32 - 1):
        full = cr.hash_priority(3000, seed)
        idx = np.array([0, 1, 17, 2998, 2999, 5, 5], np.int64)
        assert np.array_equal(cr.hash_priority_at(idx, seed), full[idx])
        assert np.array_equal(cr.hash_priority_at(np.arange(3000), seed), full)
    big = np.array([4_194_324, 2 ** 31 - 1], np.int64)
    assert cr.hash_priority_at(big, 7).tolist() == [cr.fmix32(int(v) + 7 * 0x9E3779B9) for v in big]


@pytest.mark.parametrize("symmetric", [False, True])
@pytest.mark.parametrize("name", LIFT_NAMES)
def test_graph_lifts_equal_the_plain_models(lift_graphs, name, symmetric):
    """colour, mis and aggregate on the vertices with a neighbour, lifted, against the models on the whole graph: bit for bit, the
    counts and the rounds too.  Under symmetric=True also the rounds model, which is what the device runs where the promise is false."""
    import aggref as ag
    import colourref as cr
    n, I, J, _ = lift_graphs[name]
    m = compactref.offdiag_map(n, I, J)
    assert (m.cdim < n) == (name != "ragged_37")
    cI, cJ = compactref.compact_pattern(m, I, J)
    rng = np.random.default_rng(23)
    for prio in (rng.integers(0, 2 ** 32, n).astype(np.uint32), ag.priority_array(n, "ties"), cr.hash_priority(n, 12345)):
        pc = prio[m.used]
        c, nc, rounds = cr.colouring(n, I, J, priority=prio, symmetric=symmetric)
        cc, ncc, rc = cr.colouring(m.cdim, cI, cJ, priority=pc, symmetric=symmetric)
        assert np.array_equal(compactref.lift_colours(m, cc), c) and (ncc, rc) == (nc, rounds)
        if symmetric:
            c, _, nc, rounds = cr.jones_plassmann(cr.adjacency(n, I, J, True), prio)
            cc, _, ncc, rc = cr.jones_plassmann(cr.adjacency(m.cdim, cI, cJ, True), pc)
            assert np.array_equal(compactref.lift_colours(m, cc), c) and (ncc, rc) == (nc, rounds)
        for distance in (1, 2):
            s, count, rounds = ag.mis(n, I, J, distance, priority=prio, symmetric=symmetric)
            sc, cc_, rc = ag.mis(m.cdim, cI, cJ, distance, priority=pc, symmetric=symmetric)
            ls, lcount = compactref.lift_mis(m, sc, cc_)
            assert ls.dtype == s.dtype and np.array_equal(ls, s) and (lcount, rc) == (count, rounds)
        agg, roots, nagg, rounds = ag.aggregate(n, I, J, priority=prio, symmetric=symmetric)
        ac, rootc, naggc, rc = ag.aggregate(m.cdim, cI, cJ, priority=pc, symmetric=symmetric)
        la, lr, ln = compactref.lift_aggregate(m, ac, rootc, naggc)
        assert la.dtype == agg.dtype and lr.dtype == roots.dtype
        assert np.array_equal(la, agg) and np.array_equal(lr, roots) and (ln, rc) == (nagg, rounds)
    assert np.array_equal(cr.hash_priority_at(m.used, 12345), cr.hash_priority(n, 12345)[m.used])


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=("f64", "f32"))
@pytest.mark.parametrize("name", LIFT_NAMES)
def test_solve_lifts_equal_the_plain_references(lift_graphs, name, dtype):
    """ilu0, trsv (both triangles, with and without unit_diag), lu_solve and the level schedule on the rows with an off-diagonal
    entry, lifted, against trsvref / ilu0ref on the whole system.  The upper solve needs index=: its fma order goes by the tile edge"""
    import ilu0ref
    import trsvref as tr
    n, I, J, V = lift_graphs[name]
    I, J, V, d = _with_diagonal(n, I, J, V.astype(dtype))
    V, d = V.astype(dtype), d.astype(dtype)
    m = compactref.offdiag_map(n, I, J)
    (crp, cci, cv), kept = compactref.compact_system(m, I, J, V)
    rp, ci, v = _full_csr(n, I, J, V)
    assert np.array_equal(v[kept], cv) and kept.sum() == len(cv)
    b = np.random.default_rng(29).standard_normal(n).astype(dtype)
    bc = m.gather(b)
    f, _ = ilu0ref.ilu0(n, rp, ci, v, dtype)
    fc, _ = ilu0ref.ilu0(m.cdim, crp, cci, cv, dtype)
    lifted = compactref.lift_factor(kept, fc, v)
    assert lifted.dtype == f.dtype and np.array_equal(lifted, f)
    assert ilu0ref.pivots(n, rp, ci, f)[0] == 0
    for uplo in tr.UPLO:
        for unit in (False, True):
            want = tr.trsv(n, rp, ci, v, b, uplo, unit, dtype)
            got = tr.trsv(m.cdim, crp, cci, cv, bc, uplo, unit, dtype, index=m.used)
            got = compactref.lift_solution(m, got, b, None if unit else d)
            assert got.dtype == want.dtype and np.array_equal(got, want), (uplo, unit)
        lv = tr.levels(n, rp, ci, uplo)
        lvc = tr.levels(m.cdim, crp, cci, uplo, index=m.used)
        lines = np.unique(m.used // 16)
        assert np.array_equal(lv[lines], lvc) and np.all(np.delete(lv, lines) == 1), uplo
    z = tr.trsv(n, rp, ci, f, tr.trsv(n, rp, ci, f, b, "lower", True, dtype), "upper", False, dtype)
    wc = tr.trsv(m.cdim, crp, cci, fc, bc, "lower", True, dtype, index=m.used)
    zc = tr.trsv(m.cdim, crp, cci, fc, wc, "upper", False, dtype, index=m.used)
    assert np.array_equal(compactref.lift_solution(m, zc, b, d), z), "lu_solve"
    if name == "isolated_610":     # (what index= is for: squeezing moves the tile edge, and a row's fmas change their order)
        plain = tr.trsv(m.cdim, crp, cci, cv, bc, "upper", False, dtype)
        assert not np.array_equal(plain, tr.trsv(m.cdim, crp, cci, cv, bc, "upper", False, dtype, index=m.used))
    ident = np.arange(n)
    assert np.array_equal(tr.trsv(n, rp, ci, v, b, "upper", False, dtype, index=ident), tr.trsv(n, rp, ci, v, b, "upper", False, dtype))


@pytest.mark.parametrize("name", LIFT_NAMES)
def test_arg_fold_lifts_equal_the_plain_reference(lift_graphs, name):
    """mxv_arg, reduce_arg and bfs_parents on the used lines, indices renamed back, against argref on the whole matrix"""
    import argref as ar
    n, I, J, V = lift_graphs[name]
    m = compactref.IndexMap(np.concatenate([I, J]), n)
    full, comp = _full_csr(n, I, J, V), m.csr(I, J, V)
    rng = np.random.default_rng(31)
    x, y0 = rng.standard_normal(n), rng.standard_normal(n)
    present = (rng.random(n) < 0.4).astype(np.uint8)
    i0 = np.where(rng.random(n) < 0.5, -1, m.used[rng.integers(0, m.cdim, n)]).astype(np.int32)
    i0c = np.where(m.gather(i0) >= 0, np.searchsorted(m.used, np.maximum(m.gather(i0), 0)), -1).astype(np.int32)
    for tr in (False, True):
        for kind in ar.KINDS:
            for acc in (False, True):
                old = dict(y_old=y0, idx_old=i0, accumulate=True) if acc else {}
                oldc = dict(y_old=m.gather(y0), idx_old=i0c, accumulate=True) if acc else {}
                y, idx, pres = ar.mxv_arg(n, n, *full, x, kind, np.float64, present=present, transpose=tr, **old)
                yc, idxc, presc = ar.mxv_arg(m.cdim, m.cdim, *comp, m.gather(x), kind, np.float64, present=m.gather(present), transpose=tr, **oldc)
                if y is not None:
                    assert np.array_equal(m.scatter(yc, y0 if acc else ar.START[kind]), y, equal_nan=True), (tr, kind, acc)
                got = compactref.lift_index(m, idxc, i0 if acc else -1)
                assert got.dtype == idx.dtype and np.array_equal(got, idx), (tr, kind, acc)
                assert np.array_equal(m.scatter(presc, 0), pres)
        import mxvref as mr
        for op in ("min", "max"):
            dim = "cols" if tr else "rows"
            y, idx = ar.reduce_arg(n, n, *full, op, np.float64, dim=dim)
            yc, idxc = ar.reduce_arg(m.cdim, m.cdim, *comp, op, np.float64, dim=dim)
            assert np.array_equal(m.scatter(yc, mr.IDENTITY[op]), y) and np.array_equal(compactref.lift_index(m, idxc), idx)
        for source in (int(m.used[0]), int(m.used[-1])):
            lv, par, depth, reached = ar.bfs_parents(n, full[0], full[1], source, tr)
            lvc, parc, dc, rc = ar.bfs_parents(m.cdim, comp[0], comp[1], int(np.searchsorted(m.used, source)), tr)
            assert np.array_equal(m.scatter(lvc, -1), lv) and np.array_equal(compactref.lift_index(m, parc), par)
            assert (dc, rc) == (depth, reached)


def test_hypersparse_diag_is_the_operand_of_the_solves():
    from matgen import hypersparse_diag
    n, I, J, V, S = hypersparse_diag()
    n0, I0, J0, V0, S0 = hypersparse()
    lim = 262_144
    assert n == n0 == HYPER_N and np.array_equal(S, S0) and (n + 15) // 16 < 1 << 26
    off = I != J
    assert off.sum() == (I0 != J0).sum() and np.array_equal(I[off], I0[I0 != J0]) and np.array_equal(V[off], V0[I0 != J0])
    assert np.array_equal(I[~off], np.arange(n)) and len(I) == off.sum() + n and 4_400_000 < len(I) < 4_600_000
    key = I.astype(np.int64) * n + J
    assert len(np.unique(key)) == len(key)
    assert len(np.unique((I.astype(np.int64) >> 4) * (1 << 20) + (J >> 4))) > lim
    rowsum = np.bincount(I[off], weights=np.abs(V[off]), minlength=n)
    assert np.array_equal(V[~off], 4.0 + rowsum) and np.all(V[~off] > rowsum)
    m = compactref.offdiag_map(n, I, J)
    assert lim < m.cdim < 320_000, "the references run on the rows with an off-diagonal entry"
