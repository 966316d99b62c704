"""GPU: chained products -- the C of a plan as a new tiling (pem_tiled_from_cplan) and its refresh (pem_tiled_set_values_from_cplan).

The central check: the tiling made on the device equals, array for array, the tiling the host route builds from the plan's
export (pem_c_export_csr + pem_tiled_from_csr; for C^T, pem_c_export_coo + pem_tiled_from_coo(transpose = 1)).  Chains are checked
against the CPU oracle applied twice (plus-times, bit for bit) and against semiringref (min_plus, lor_land).
"""
import numpy as np
import pytest
import torch

import chainref
import semiringref as sr
from matgen import _vals, cases

pytestmark = pytest.mark.gpu

torch.cuda.is_available()   # (torch's runtime first, as in the other GPU files)

CASES = cases()
PEM_E_INVALID, PEM_E_STATE = -1, -6
DTYPES = (np.float64, np.float32)
INFO = ("rows", "cols", "nnz", "tile_rows", "tile_cols", "ntiles", "value_bytes")


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32) if a.dtype.kind == "f" else a


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _tilings(pkg, ctx, case, dtype=np.float64, V=None):
    rows, cols, I, J, V0, tr = case
    V = V0 if V is None else V
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=dtype)
    B = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, True, dtype=dtype) if tr else A
    return A, B


def _reconvert(pkg, ctx, plan, transpose):
    """today's route: export C, convert it again"""
    rows, cols, dt = plan.A.rows, plan.B.cols, plan.A.dtype
    if transpose:
        r, c, v = plan.export_coo()
        return pkg.Tiled.from_coo(ctx, rows, cols, r, c, v, True, dtype=dt)
    i = plan.info()
    rp, ci, v = plan.export_csr()
    full = np.full(rows + 1, rp[-1], np.int32)           # the export's row pointer is relative to the plan's row slice
    full[:i["row_begin"] + 1] = 0
    full[i["row_begin"]:i["row_end"] + 1] = rp
    return pkg.Tiled.from_csr(ctx, rows, cols, full, ci, v, dtype=dt)


def _assert_same_tiling(got, want, label):
    for k in INFO:
        assert getattr(got, k) == getattr(want, k), f"{label}: {k} {getattr(got, k)} != {getattr(want, k)}"
    for name in ("tile_keys", "tile_nnz_ptr", "masks", "rowptr", "rowcolidx", "vals", "masks_t", "tile_rowptr", "tile_colidx",
                 "tile_colptr", "tile_rowidx", "tile_offsets"):
        assert _same(got.array(name), want.array(name)), f"{label}: array {name} differs"


def _check_equal(pkg, ctx, plan, label):
    for tr in (0, 1):
        got = pkg.Tiled.from_cplan(plan, transpose=tr)
        want = _reconvert(pkg, ctx, plan, tr)
        _assert_same_tiling(got, want, f"{label} transpose={tr}")
        got.close()
        want.close()


# ---- equality with export + reconvert ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", sorted(CASES))
def test_equals_reconvert_every_case(pkg, ctx, name, dtype):
    A, B = _tilings(pkg, ctx, CASES[name], dtype)
    plan = pkg.CPlan(ctx, A, B)
    plan.spgemm()
    _check_equal(pkg, ctx, plan, name)


def test_matches_numpy_restatement(pkg, ctx):
    """chainref (the CPU tests' restatement) on the plan's own C arrays gives the device's payload"""
    for name in ("rand_300", "band_1500", "rect_70x40_AAt", "powerlaw_600"):
        A, B = _tilings(pkg, ctx, CASES[name])
        plan = pkg.CPlan(ctx, A, B)
        plan.set_option("prune", 0)
        plan.spgemm()
        c = {k: plan.array(k) for k in ("c_tile_rowidx", "c_tile_colidx", "c_mask", "c_tile_nnz_ptr", "c_vals")}
        for tr in (False, True):
            want = chainref.payload(c, A.rows, B.cols, transpose=tr)
            T = pkg.Tiled.from_cplan(plan, tr)
            for k in ("tile_keys", "tile_nnz_ptr", "rowcolidx", "vals"):
                assert _same(T.array(k), want[k]), (name, tr, k)


@pytest.mark.parametrize("option", ("prune", "wide"))
@pytest.mark.parametrize("name", ("rand_300", "band_1500", "rect_33x65_AAt", "blockrows_1600", "cancel_and_zero"))
def test_equals_reconvert_options(pkg, ctx, name, option):
    A, B = _tilings(pkg, ctx, CASES[name])
    plan = pkg.CPlan(ctx, A, B)
    plan.set_option(option, 0)
    plan.spgemm()
    if option == "prune":
        assert plan.info()["ntiles_c"] >= pkg.Tiled.from_cplan(plan).ntiles
    _check_equal(pkg, ctx, plan, f"{name} {option}=0")


def _tile_emptying_mask(pkg, ctx, plan, dtype):
    """a mask that keeps C's pattern in every other C tile and, in the others, one position C does not hold (where there is one):
    the masked plan then lists tiles without entries"""
    r, c, _ = plan.export_coo()
    rows, cols = plan.A.rows, plan.B.cols
    held = set(zip(r.tolist(), c.tolist()))
    tiles = sorted({(i >> 4, j >> 4) for i, j in held})
    MI, MJ = [], []
    for k, (ti, tj) in enumerate(tiles):
        if k % 2 == 0:
            cells = [(i, j) for i, j in held if i >> 4 == ti and j >> 4 == tj]
        else:
            cells = [(i, j) for i in range(16 * ti, min(16 * ti + 16, rows)) for j in range(16 * tj, min(16 * tj + 16, cols))
                     if (i, j) not in held][:1]
        for i, j in cells:
            MI.append(i)
            MJ.append(j)
    return pkg.Tiled.from_coo(ctx, rows, cols, np.array(MI, np.int32), np.array(MJ, np.int32), np.ones(len(MI)), dtype=dtype)


@pytest.mark.parametrize("complement", (False, True), ids=("structure", "complement"))
@pytest.mark.parametrize("name", ("rand_300", "band_1500", "rect_70x40_AAt", "dense_48"))
def test_equals_reconvert_masked(pkg, ctx, name, complement):
    A, B = _tilings(pkg, ctx, CASES[name])
    full = pkg.CPlan(ctx, A, B)
    full.spgemm()
    for M in (A if A.cols == B.cols else _tile_emptying_mask(pkg, ctx, full, np.float64), _tile_emptying_mask(pkg, ctx, full, np.float64),
              pkg.Tiled.from_cplan(full)):
        plan = pkg.CPlan(ctx, A, B, mask=M, complement=complement)
        plan.spgemm()
        _check_equal(pkg, ctx, plan, f"{name} masked complement={complement}")
    # the complement of C's own pattern: every C tile stays listed, none holds an entry
    own = pkg.Tiled.from_cplan(full)
    plan = pkg.CPlan(ctx, A, B, mask=own, complement=True)
    plan.spgemm()
    T = pkg.Tiled.from_cplan(plan)
    assert T.nnz == 0 and T.ntiles == 0
    _check_equal(pkg, ctx, plan, f"{name} complement of own pattern")


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", ("rand_300", "band_1500", "empty_rows", "rect_70x40_AAt", "hub_row_4000"))
def test_equals_reconvert_row_ranges(pkg, ctx, name, dtype):
    A, B = _tilings(pkg, ctx, CASES[name], dtype)
    mt = A.tile_rows
    for lo, hi in ((0, mt // 2), (mt // 3, mt), (mt // 3, mt // 3 + 1)):
        plan = pkg.CPlan(ctx, A, B, lo, hi)
        plan.spgemm()
        T = pkg.Tiled.from_cplan(plan)
        assert (T.rows, T.cols) == (A.rows, B.cols)
        keys = T.array("tile_keys") >> 32
        assert np.all((keys >= lo) & (keys < hi)), (lo, hi)
        _check_equal(pkg, ctx, plan, f"{name} rows [{lo}, {hi})")


@pytest.mark.parametrize("semiring", ("plus_times", "min_plus", "max_plus", "max_times", "plus_pair", "lor_land"))
def test_equals_reconvert_semirings(pkg, ctx, semiring):
    for name in ("rand_300", "band_1500", "rect_33x65_AAt"):
        for dt in DTYPES:
            A, B = _tilings(pkg, ctx, CASES[name], dt)
            plan = pkg.CPlan(ctx, A, B, semiring=semiring)
            plan.spgemm()
            _check_equal(pkg, ctx, plan, f"{name} {semiring}")


# ---- chains ----------------------------------------------------------------------------------------------------------------
def _oracle_chain(oracle, case, f32, order):
    """plus-times products by the oracle; order 'left': (A A) A, 'right': A (A A)"""
    rows, cols, I, J, V, _ = case
    if f32:
        V = V.astype(np.float32).astype(np.float64)
    a = oracle.Csr(rows, cols, I, J, V)
    c1 = oracle.csr_spgemm(a, a, f32=f32)
    rp, ci, v = c1.arrays()
    r = np.repeat(np.arange(rows, dtype=np.int32), np.diff(rp))
    c1c = oracle.Csr(rows, cols, r, ci, v)
    out = oracle.csr_spgemm(c1c, a, f32=f32) if order == "left" else oracle.csr_spgemm(a, c1c, f32=f32)
    return out.arrays()


def _check_csr(got, want, label):
    rp, ci, v = got
    wrp, wci, wv = want
    assert np.array_equal(rp, wrp) and np.array_equal(ci, wci), f"{label}: structure"
    assert _same(v, np.asarray(wv).astype(v.dtype)), f"{label}: values"


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", ("rand_50", "rand_300", "band_1500", "powerlaw_600", "ragged_37", "dense_48", "cancel_and_zero", "empty_matrix"))
def test_cube_left_and_right(pkg, oracle, ctx, name, dtype):
    case = CASES[name]
    A, _ = _tilings(pkg, ctx, case, dtype)
    p1 = pkg.CPlan(ctx, A, A)
    p1.spgemm()
    C1 = pkg.Tiled.from_cplan(p1)
    left = pkg.CPlan(ctx, C1, A)
    left.spgemm()
    right = pkg.CPlan(ctx, A, C1)
    right.spgemm()
    f32 = dtype == np.float32
    _check_csr(left.export_csr(), _oracle_chain(oracle, case, f32, "left"), f"{name} (AA)A")
    _check_csr(right.export_csr(), _oracle_chain(oracle, case, f32, "right"), f"{name} A(AA)")


@pytest.mark.parametrize("name", ("rect_70x40_AAt", "rect_33x65_AAt", "banded_500_AAt", "rand_300"))
def test_transposed_c_as_operand(pkg, oracle, ctx, name):
    """C = A B, then C^T C (C^T from the device) against the oracle's C^T C"""
    rows, cols, I, J, V, tr = CASES[name]
    A, B = _tilings(pkg, ctx, CASES[name])
    p1 = pkg.CPlan(ctx, A, B)
    p1.spgemm()
    Ct, Cn = pkg.Tiled.from_cplan(p1, transpose=True), pkg.Tiled.from_cplan(p1)
    p2 = pkg.CPlan(ctx, Ct, Cn)
    p2.spgemm()
    r, c, v = p1.export_coo()
    oc = oracle.Csr(A.rows, B.cols, r, c, v)
    oct_ = oracle.Csr(A.rows, B.cols, r, c, v, True)
    _check_csr(p2.export_csr(), oracle.csr_spgemm(oct_, oc).arrays(), f"{name} C^T C")


@pytest.mark.parametrize("name", ("rand_300", "band_1500", "powerlaw_600"))
def test_c_as_mask(pkg, ctx, name):
    """(A A)<A A>: masked by its own pattern it is A A; the complement is empty.  A A A<A A>: the filter of A^3 by C's pattern."""
    A, _ = _tilings(pkg, ctx, CASES[name])
    p1 = pkg.CPlan(ctx, A, A)
    p1.spgemm()
    M = pkg.Tiled.from_cplan(p1)
    own = pkg.CPlan(ctx, A, A, mask=M)
    own.spgemm()
    for x, y in zip(own.export_csr(), p1.export_csr()):
        assert _same(x, y)
    comp = pkg.CPlan(ctx, A, A, mask=M, complement=True)
    comp.spgemm()
    assert comp.info()["nnz_c"] == 0
    cube = pkg.CPlan(ctx, M, A)
    cube.spgemm()
    masked = pkg.CPlan(ctx, M, A, mask=M)
    masked.spgemm()
    r3, c3, v3 = cube.export_coo()
    r2, c2, _ = p1.export_coo()
    keep = np.isin(r3.astype(np.int64) * A.cols + c3, r2.astype(np.int64) * A.cols + c2)
    rm, cm, vm = masked.export_coo()
    assert np.array_equal(rm, r3[keep]) and np.array_equal(cm, c3[keep]) and _same(vm, v3[keep])


@pytest.mark.parametrize("semiring", ("min_plus", "lor_land"))
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_semiring_chains(pkg, ctx, semiring, dtype):
    for name in ("rand_300", "band_1500", "powerlaw_600"):
        rows, cols, I, J, V, _ = CASES[name]
        Vs = np.abs(V) if semiring == "min_plus" else V
        A, _ = _tilings(pkg, ctx, CASES[name], dtype, Vs)
        p1 = pkg.CPlan(ctx, A, A, semiring=semiring)
        p1.spgemm()
        C1 = pkg.Tiled.from_cplan(p1)
        p2 = pkg.CPlan(ctx, C1, A, semiring=semiring)
        p2.spgemm()
        a = sr.coo_to_csr(rows, cols, I, J, Vs)
        c1 = sr.spgemm(a, a, cols, semiring, dtype)
        want = sr.spgemm(c1, a, cols, semiring, dtype)
        rp, ci, v = p2.export_csr()
        assert np.array_equal(rp, want[0]) and np.array_equal(ci, want[1]), (name, semiring)
        assert sr.same_values(v, want[2]), (name, semiring)


def _aggregation(n, size=16):
    """P (n x ceil(n/size)): row i -> aggregate i // size, value 1"""
    I = np.arange(n, dtype=np.int32)
    return n, (n + size - 1) // size, I, (I // size).astype(np.int32), np.ones(n)


def test_galerkin(pkg, oracle, ctx):
    rows, cols, I, J, V, _ = CASES["banded_500_AAt"]
    pn, pc, PI, PJ, PV = _aggregation(rows)
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    P = pkg.Tiled.from_coo(ctx, pn, pc, PI, PJ, PV)
    Pt = pkg.Tiled.from_coo(ctx, pn, pc, PI, PJ, PV, True)
    ap = pkg.CPlan(ctx, A, P)
    ap.spgemm()
    AP = pkg.Tiled.from_cplan(ap)
    g = pkg.CPlan(ctx, Pt, AP)
    g.spgemm()
    oa, op, opt = oracle.Csr(rows, cols, I, J, V), oracle.Csr(pn, pc, PI, PJ, PV), oracle.Csr(pn, pc, PI, PJ, PV, True)
    oap = oracle.csr_spgemm(oa, op)
    _check_csr(g.export_csr(), oracle.csr_spgemm(opt, oap).arrays(), "P^T (A P)")


# ---- refresh ---------------------------------------------------------------------------------------------------------------
def _csr_order(I, J):
    return np.argsort(I.astype(np.int64) * (int(J.max()) + 1 if len(J) else 1) + J, kind="stable")


@pytest.mark.parametrize("transpose", (0, 1))
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_refresh_through_the_chain(pkg, ctx, transpose, dtype):
    for name in ("band_1500", "rand_300", "rect_70x40_AAt"):
        case = CASES[name]
        rows, cols, I, J, V, tr = case
        A, B = _tilings(pkg, ctx, case, dtype)
        p1 = pkg.CPlan(ctx, A, B)
        p1.spgemm()
        T = pkg.Tiled.from_cplan(p1, transpose)
        p2 = pkg.CPlan(ctx, T, T if transpose == 0 and T.rows == T.cols else pkg.Tiled.from_cplan(p1, 1 - transpose))
        p2.spgemm()
        for seed in (5, 6):
            V2 = _vals(np.random.default_rng(seed), len(I))
            o = _csr_order(I, J)
            A.set_values(V2[o], "row")
            if tr:
                B.set_values(V2[o], "col")
            with pytest.raises(pkg.PemError) as e:        # C of p1 is stale until its step 3
                T.set_values_from_cplan(p1)
            assert e.value.status == PEM_E_STATE
            p1.step3()
            T.set_values_from_cplan(p1)
            if p2.B is not T:
                p2.B.set_values_from_cplan(p1)
            with pytest.raises(pkg.PemError) as e:        # p2 is stale until its step 3
                p2.export_csr()
            assert e.value.status == PEM_E_STATE
            p2.step3()
            A2, B2 = _tilings(pkg, ctx, case, dtype, V2)
            f1 = pkg.CPlan(ctx, A2, B2)
            f1.spgemm()
            F = pkg.Tiled.from_cplan(f1, transpose)
            _assert_same_tiling(T, F, f"{name} refreshed T")
            f2 = pkg.CPlan(ctx, F, F if p2.B is T else pkg.Tiled.from_cplan(f1, 1 - transpose))
            f2.spgemm()
            for x, y in zip(p2.export_csr(), f2.export_csr()):
                assert _same(x, y), (name, seed)


def test_refresh_valid_after_options_and_semiring(pkg, ctx):
    A, _ = _tilings(pkg, ctx, CASES["band_1500"])
    p = pkg.CPlan(ctx, A, A)
    p.spgemm()
    T = pkg.Tiled.from_cplan(p, 1)
    p.set_option("prune", 0)
    p.set_semiring("max_plus")
    with pytest.raises(pkg.PemError) as e:
        T.set_values_from_cplan(p)
    assert e.value.status == PEM_E_STATE
    p.spgemm()
    T.set_values_from_cplan(p)
    _assert_same_tiling(T, pkg.Tiled.from_cplan(p, 1), "after set_option + set_semiring")


def test_refresh_errors(pkg, ctx):
    A, _ = _tilings(pkg, ctx, CASES["rand_300"])
    p = pkg.CPlan(ctx, A, A)
    p.spgemm()
    q = pkg.CPlan(ctx, A, A)
    q.spgemm()
    T = pkg.Tiled.from_cplan(p)
    for t, plan in ((T, q), (A, p)):                      # a tiling of another plan; a user-built tiling
        with pytest.raises(pkg.PemError) as e:
            t.set_values_from_cplan(plan)
        assert e.value.status == PEM_E_INVALID
    p.close()                                             # a plan created after it (possibly at the same address)
    for _ in range(4):
        r = pkg.CPlan(ctx, A, A)
        r.spgemm()
        with pytest.raises(pkg.PemError) as e:
            T.set_values_from_cplan(r)
        assert e.value.status == PEM_E_INVALID
        r.close()


def test_graph_replay_picks_up_the_refresh(pkg, ctx):
    case = CASES["band_1500"]
    rows, cols, I, J, V, _ = case
    g = pkg.Context(0)
    try:
        g.set_graph_replay(True)
        A, _ = _tilings(pkg, g, case)
        p1 = pkg.CPlan(g, A, A)
        p1.spgemm()
        T = pkg.Tiled.from_cplan(p1)
        p2 = pkg.CPlan(g, T, A)
        for _ in range(3):
            p2.spgemm()                                   # captured, then replayed
        for seed in (21, 22, 23):
            V2 = _vals(np.random.default_rng(seed), len(I))
            A.set_values(V2[_csr_order(I, J)])
            p1.step3()
            T.set_values_from_cplan(p1)
            p2.spgemm()
            A2, _ = _tilings(pkg, ctx, case, V=V2)
            f1 = pkg.CPlan(ctx, A2, A2)
            f1.spgemm()
            F = pkg.Tiled.from_cplan(f1)
            f2 = pkg.CPlan(ctx, F, A2)
            f2.spgemm()
            for x, y in zip(p2.export_csr(), f2.export_csr()):
                assert _same(x, y), seed
    finally:
        g.close()


# ---- independence ----------------------------------------------------------------------------------------------------------
def test_outlives_the_plan_and_round_trips_the_cache(pkg, ctx, tmp_path):
    A, _ = _tilings(pkg, ctx, CASES["powerlaw_600"])
    p = pkg.CPlan(ctx, A, A)
    p.spgemm()
    want = _reconvert(pkg, ctx, p, 0)
    T = pkg.Tiled.from_cplan(p)
    p.set_option("prune", 0)
    p.spgemm()
    p.close()
    _assert_same_tiling(T, want, "after the plan is gone")
    q = pkg.CPlan(ctx, T, A)
    q.spgemm()
    r = pkg.CPlan(ctx, want, A)
    r.spgemm()
    for x, y in zip(q.export_csr(), r.export_csr()):
        assert _same(x, y)
    assert pkg.flop_count(ctx, T, A) == pkg.flop_count(ctx, want, A)
    assert np.array_equal(pkg.split_tile_rows(ctx, T, A, 3), pkg.split_tile_rows(ctx, want, A, 3))
    path = str(tmp_path / "c.pemt")
    T.save(path)
    _assert_same_tiling(pkg.Tiled.load(ctx, path), want, "save / load")
    V2 = _vals(np.random.default_rng(9), T.nnz)
    T.set_values(V2)
    want.set_values(V2)
    _assert_same_tiling(T, want, "set_values")


def test_memory_flat_over_create_destroy(pkg):
    g = pkg.Context(0)
    try:
        A, _ = _tilings(pkg, g, CASES["band_1500"])
        seen = []
        for k in range(6):
            p = pkg.CPlan(g, A, A)
            p.spgemm()
            for tr in (0, 1):
                T = pkg.Tiled.from_cplan(p, tr)
                T.set_values_from_cplan(p)
                g.synchronize()
                T.close()
            p.close()
            seen.append(g.memory_stats()["in_use_bytes"])
        assert len(set(seen[1:])) == 1, seen
    finally:
        g.close()


# ---- errors, empty, full size ----------------------------------------------------------------------------------------------
def test_errors(pkg, ctx):
    import ctypes as C
    A, _ = _tilings(pkg, ctx, CASES["rand_300"])
    p = pkg.CPlan(ctx, A, A)
    for step in (None, p.step1, p.step2):                # before step 3
        if step:
            step()
        with pytest.raises(pkg.PemError) as e:
            pkg.Tiled.from_cplan(p)
        assert e.value.status == PEM_E_STATE
    p.step3()
    pkg.Tiled.from_cplan(p).close()
    for bad in (2, -1):
        with pytest.raises(pkg.PemError) as e:
            pkg.Tiled.from_cplan(p, bad)
        assert e.value.status == PEM_E_INVALID
    L, h = pkg.lib(), C.c_void_p()
    assert L.pem_tiled_from_cplan(None, p._h, 0, C.byref(h)) == PEM_E_INVALID
    assert L.pem_tiled_from_cplan(ctx._h, None, 0, C.byref(h)) == PEM_E_INVALID
    assert L.pem_tiled_from_cplan(ctx._h, p._h, 0, None) == PEM_E_INVALID
    assert L.pem_tiled_set_values_from_cplan(ctx._h, None, p._h) == PEM_E_INVALID
    A.set_values(A.array("vals"))                         # a refresh of A: C is stale
    with pytest.raises(pkg.PemError) as e:
        pkg.Tiled.from_cplan(p)
    assert e.value.status == PEM_E_STATE
    p.step3()
    p.set_semiring("min_plus")
    with pytest.raises(pkg.PemError) as e:
        pkg.Tiled.from_cplan(p)
    assert e.value.status == PEM_E_STATE


def test_empty_c_is_a_valid_operand(pkg, ctx):
    for name in ("empty_matrix", "empty_rows"):
        rows, cols, I, J, V, _ = CASES[name]
        A, _ = _tilings(pkg, ctx, CASES[name])
        Z = pkg.Tiled.from_coo(ctx, rows, cols, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
        p = pkg.CPlan(ctx, Z, A)
        p.spgemm()
        for tr in (0, 1):
            T = pkg.Tiled.from_cplan(p, tr)
            assert T.nnz == 0 and T.ntiles == 0 and (T.rows, T.cols) == ((rows, cols) if tr == 0 else (cols, rows))
            T.set_values_from_cplan(p)
            q = pkg.CPlan(ctx, T, A)
            q.spgemm()
            assert q.info()["nnz_c"] == 0
        _check_equal(pkg, ctx, p, name)


def test_full_size_webbase(pkg, standins, ctx):
    rows, cols, I, J, V = standins.make("webbase-1M", 1.0)
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    p = pkg.CPlan(ctx, A, A)
    p.spgemm()
    for tr in (0, 1):
        got = pkg.Tiled.from_cplan(p, tr)
        want = _reconvert(pkg, ctx, p, tr)
        _assert_same_tiling(got, want, f"webbase-1M A^2 transpose={tr}")
        got.close()
        want.close()
