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
