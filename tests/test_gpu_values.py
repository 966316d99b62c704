"""GPU: numeric refresh -- new values written into existing tilings (pem_tiled_set_values*), C recomputed by step 3 alone.

Every check compares against a fresh pipeline built directly on the new values (conversion, plan, steps 1-3): the refreshed
tiling's arrays and the recomputed C must equal it bit for bit, and C the CPU oracle's.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from matgen import _vals, cases

pytestmark = pytest.mark.gpu

# torch's device runtime comes up before the library opens the device (the session's `ctx` fixture): the other way round,
# torch found no GPU in the process when this file ran on its own.  (Collection imports every module before any test runs.)
torch.cuda.is_available()

CASES = cases()
PEM_E_INVALID, PEM_E_STATE = -1, -6


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32) if a.dtype.kind == "f" else a


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def csr_order(I, J):
    """source entry indices in (row, col) order: V[csr_order(I, J)] is the CSR-ordered value array"""
    return np.argsort(I.astype(np.int64) * (int(J.max()) + 1 if len(J) else 1) + J, kind="stable")


def _results(plan):
    return [*plan.export_csr(), *plan.export_coo(), plan.array("c_vals")]


def _tilings(pkg, ctx, case, V, dtype=np.float64):
    rows, cols, I, J, _, tr = case
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=dtype)
    B = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, True, dtype=dtype) if tr else A
    return A, B


def _fresh(pkg, ctx, case, V, dtype=np.float64, options=()):
    A, B = _tilings(pkg, ctx, case, V, dtype)
    plan = pkg.CPlan(ctx, A, B)
    for k, v in options:
        plan.set_option(k, v)
    plan.spgemm()
    return A, B, plan


def _refresh_and_compare(pkg, oracle, ctx, name, dtype=np.float64, options=(), check_oracle=True):
    case = CASES[name]
    rows, cols, I, J, V, tr = case
    V2src = _vals(np.random.default_rng(777), len(I))
    V2 = V2src[csr_order(I, J)]                           # CSR order of A = column-major order of the A^T tiling
    A, B = _tilings(pkg, ctx, case, V, dtype)
    plan = pkg.CPlan(ctx, A, B)
    for k, v in options:
        plan.set_option(k, v)
    plan.spgemm()
    A.set_values(V2, "row")
    if tr:
        B.set_values(V2, "col")
    plan.step3()
    A2, B2, plan2 = _fresh(pkg, ctx, case, V2src, dtype, options)
    assert _same(A.array("vals"), A2.array("vals")), f"{name}: refreshed A vals"
    assert _same(B.array("vals"), B2.array("vals")), f"{name}: refreshed B vals"
    for k, (g, w) in enumerate(zip(_results(plan), _results(plan2))):
        assert _same(g, w), f"{name} {options}: result {k} differs from a fresh pipeline on the new values"
    if check_oracle and dtype == np.float64:
        sa, sb = oracle.Csr(rows, cols, I, J, V2src, False), oracle.Csr(rows, cols, I, J, V2src, tr)
        rp, ci, v = plan.export_csr()
        rp1, ci1, v1 = oracle.csr_spgemm(sa, sb).arrays()
        assert np.array_equal(rp, rp1) and np.array_equal(ci, ci1) and np.array_equal(v, v1), f"{name}: against the oracle"
    return plan


@pytest.mark.parametrize("name", list(CASES))
def test_refresh_then_step3_equals_fresh_pipeline(pkg, oracle, ctx, name):
    """(dense_48's COO input is permuted, so its map is no identity; the AAt cases refresh A^T with the same array, "col")"""
    _refresh_and_compare(pkg, oracle, ctx, name)


def test_distinct_rectangular_operands_refreshed_alone_and_together(pkg, oracle, ctx):
    rng = np.random.default_rng(31)
    m, k, n = 70, 53, 90
    ka = rng.choice(m * k, 900, replace=False)
    kb = rng.choice(k * n, 1300, replace=False)
    AI, AJ, BI, BJ = (ka // k).astype(np.int32), (ka % k).astype(np.int32), (kb // n).astype(np.int32), (kb % n).astype(np.int32)
    AV1, BV1, AV2, BV2 = _vals(rng, 900), _vals(rng, 1300), _vals(rng, 900), _vals(rng, 1300)
    for which in ("A", "B", "AB"):
        A = pkg.Tiled.from_coo(ctx, m, k, AI, AJ, AV1)
        B = pkg.Tiled.from_coo(ctx, k, n, BI, BJ, BV1)
        plan = pkg.CPlan(ctx, A, B)
        plan.spgemm()
        av = AV2 if "A" in which else AV1
        bv = BV2 if "B" in which else BV1
        if "A" in which:
            A.set_values(AV2[csr_order(AI, AJ)])
        if "B" in which:
            B.set_values(BV2[csr_order(BI, BJ)], "row")
        plan.step3()
        fa, fb = pkg.Tiled.from_coo(ctx, m, k, AI, AJ, av), pkg.Tiled.from_coo(ctx, k, n, BI, BJ, bv)
        fresh = pkg.CPlan(ctx, fa, fb)
        fresh.spgemm()
        for g, w in zip(_results(plan), _results(fresh)):
            assert _same(g, w), which
        rp, ci, v = oracle.csr_spgemm(oracle.Csr(m, k, AI, AJ, av), oracle.Csr(k, n, BI, BJ, bv)).arrays()
        got = plan.export_csr()
        assert np.array_equal(got[0], rp) and np.array_equal(got[1], ci) and np.array_equal(got[2], v), which


VARIANTS = [(("wide", 0),), (("wide", 1),), (("s3_band", 1),), (("s3_band", 0),), (("s3_decode", 0),), (("s2_transposed", 1),)]


@pytest.mark.parametrize("options", VARIANTS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o))
@pytest.mark.parametrize("name", ["powerlaw_600", "dense_48", "rect_70x40_AAt", "band_1500", "hub_row_4000"])
def test_refresh_under_every_step3_reader(pkg, oracle, ctx, name, options):
    """the baseline kernels read B->vals, the entry-per-lane and band kernels B->vals_t: both layouts must be refreshed"""
    _refresh_and_compare(pkg, oracle, ctx, name, options=options)


@pytest.mark.parametrize("name", ["powerlaw_600", "rect_70x40_AAt", "dense_48", "band_1500"])
def test_refresh_fp32(pkg, oracle, ctx, name):
    _refresh_and_compare(pkg, oracle, ctx, name, dtype=np.float32)


def test_special_values_survive_bit_for_bit(pkg, oracle, ctx):
    case = CASES["dense_48"]
    rows, cols, I, J, V, tr = case
    n = len(I)
    bits = _vals(np.random.default_rng(5), n).view(np.uint64).copy()
    specials = np.array([0x7FF8_0000_DEAD_BEEF, 0xFFF8_0000_0000_1234, 0x7FF4_0000_0000_0001, 0x7FF0_0000_0000_0000,
                         0xFFF0_0000_0000_0000, 0x8000_0000_0000_0000, 0x0000_0000_0000_0001, 0x800F_FFFF_FFFF_FFFF,
                         0x0000_0000_0000_0000], np.uint64)
    bits[:: n // len(specials)][: len(specials)] = specials
    V2src = bits.view(np.float64)
    A, _ = _tilings(pkg, ctx, case, V)
    plan = pkg.CPlan(ctx, A, A)
    plan.spgemm()
    A.set_values(V2src[csr_order(I, J)])
    plan.step3()
    A2, _, plan2 = _fresh(pkg, ctx, case, V2src)
    got = A.array("vals").view(np.uint64)
    assert np.array_equal(got, A2.array("vals").view(np.uint64))
    assert set(specials.tolist()) <= set(got.tolist())
    for g, w in zip(_results(plan), _results(plan2)):   # (vals_t went through step 3: same bits in, same bits out)
        assert _same(g, w)
    # fp32
    fb = (_vals(np.random.default_rng(6), n).astype(np.float32)).view(np.uint32).copy()
    fs = np.array([0x7FC0_BEEF, 0xFFA0_0001, 0x7F80_0000, 0xFF80_0000, 0x8000_0000, 0x0000_0001, 0x807F_FFFF], np.uint32)
    fb[:: n // len(fs)][: len(fs)] = fs
    F = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=np.float32)
    F.set_values(fb.view(np.float32)[csr_order(I, J)])
    F2 = pkg.Tiled.from_coo(ctx, rows, cols, I, J, fb.view(np.float32), dtype=np.float32)
    assert np.array_equal(F.array("vals").view(np.uint32), F2.array("vals").view(np.uint32))
    assert set(fs.tolist()) <= set(F.array("vals").view(np.uint32).tolist())


def test_stale_values_refuse_export_until_step3(pkg, oracle, ctx):
    case = CASES["powerlaw_600"]
    rows, cols, I, J, V, tr = case
    A, _, plan = _fresh(pkg, ctx, case, V)
    other_A, _, other = _fresh(pkg, ctx, CASES["rand_300"], CASES["rand_300"][4])
    before = {k: plan.array(k) for k in ("pairs_a", "pairs_b", "c_mask", "c_tile_nnz_ptr", "pairs_offset", "c_tile_colidx")}
    A.set_values(_vals(np.random.default_rng(9), len(I)))
    nz, nrows = plan.info()["nnz_c"], rows
    dr, dc, dv = (torch.zeros(nrows + 1, dtype=torch.int32, device="cuda"), torch.zeros(nz, dtype=torch.int32, device="cuda"),
                  torch.zeros(nz, dtype=torch.float64, device="cuda"))
    for call in (plan.export_csr, plan.export_coo, lambda: plan.array("c_vals"),
                 lambda: plan.export_csr_device(dr.data_ptr(), dc.data_ptr(), dv.data_ptr())):
        with pytest.raises(pkg.PemError) as e:
            call()
        assert e.value.status == PEM_E_STATE and "set_values" in str(e.value)
    for k, v in before.items():                          # the symbolic arrays stay readable (and unchanged)
        assert np.array_equal(plan.array(k), v), k
    assert other.export_csr()[0].shape == (301,)         # a plan over other tilings is unaffected
    plan.step3()
    assert len(plan.export_csr()[2]) == nz and len(plan.array("c_vals")) == nz
    # B's refresh counts too (here A is B), and a full pem_spgemm makes C current as well
    A.set_values(_vals(np.random.default_rng(10), len(I)))
    with pytest.raises(pkg.PemError):
        plan.export_coo()
    plan.spgemm()
    plan.export_coo()


def test_graph_replay_picks_up_refreshed_values(pkg, oracle, ctx):
    case = CASES["band_1500"]
    rows, cols, I, J, V, tr = case
    order = csr_order(I, J)
    g = pkg.Context(0)
    try:
        g.set_graph_replay(True)
        A, _ = _tilings(pkg, g, case, V)
        plan = pkg.CPlan(g, A, A)
        plan.spgemm()
        plan.spgemm()                                     # repeat pass: captured and replayed
        plan.spgemm()
        allocs = []
        for seed in (2, 3, 4):
            Vn = _vals(np.random.default_rng(seed), len(I))
            A.set_values(Vn[order])
            plan.spgemm()
            allocs.append(g.memory_stats()["driver_allocs"])
            _, _, fresh = _fresh(pkg, ctx, case, Vn)      # (on another context: its allocations are not counted)
            for x, y in zip(_results(plan), _results(fresh)):
                assert _same(x, y), seed
        assert allocs[1] == allocs[0] and allocs[2] == allocs[0], allocs
    finally:
        g.close()


def test_device_form_from_torch_reads_nothing_back(pkg, oracle):
    case = CASES["rect_70x40_AAt"]
    rows, cols, I, J, V, tr = case
    stream = torch.cuda.Stream()                          # (not the null stream: the context would make its own)
    g = pkg.Context(0, stream=stream.cuda_stream)
    try:
        torch.cuda.set_stream(stream)
        g.reserve(64 << 20)
        A, B = _tilings(pkg, g, case, V)
        plan = pkg.CPlan(g, A, B)
        plan.spgemm()
        for seed in (11, 12):                             # first call (maps built), then the steady state
            Vn = _vals(np.random.default_rng(seed), len(I))
            dV = torch.from_numpy(Vn[csr_order(I, J)]).to("cuda")
            torch.cuda.synchronize()
            torch.cuda._sleep(200_000_000)                # ~0.1 s of GPU work ahead of the refresh on the same stream
            A.set_values_device(dV, "row")
            B.set_values_device(dV, order="col")
            assert not stream.query(), "set_values_device waited for the stream"
            g.synchronize()
            plan.step3()
            _, _, fresh = _fresh(pkg, g, case, Vn)
            for x, y in zip(_results(plan), _results(fresh)):
                assert _same(x, y), seed
        with pytest.raises(ValueError):
            A.set_values_device(dV.to(torch.float32))
        with pytest.raises(ValueError):
            A.set_values_device(dV[:-1])
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream())
        g.close()


def _full_size(pkg, ctx, rows, cols, I, J, V, lo=0, hi=-1):
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    plan = pkg.CPlan(ctx, A, A, lo, hi)
    plan.spgemm()
    return A, plan


def test_full_size_webbase_refresh_and_row_blocks(pkg, standins, ctx):
    rows, cols, I, J, V = standins.make("webbase-1M", 1.0)
    order = csr_order(I, J)
    V2 = _vals(np.random.default_rng(21), len(I))
    A, plan = _full_size(pkg, ctx, rows, cols, I, J, V)
    bounds = pkg.split_tile_rows(ctx, A, A, 3)
    blocks = [pkg.CPlan(ctx, A, A, int(bounds[p]), int(bounds[p + 1])) for p in range(3)]
    for b in blocks:
        b.spgemm()
    A.set_values(V2[order])
    plan.step3()
    got = plan.export_csr()
    _, fresh = _full_size(pkg, ctx, rows, cols, I, J, V2)
    want = fresh.export_csr()
    for x, y in zip(got, want):
        assert np.array_equal(x, y)
    parts = []
    for b in blocks:
        b.step3()
        parts.append(b.export_csr())
    rp = np.concatenate([parts[0][0]] + [p[0][1:] + sum(len(q[1]) for q in parts[:k + 1]) for k, p in enumerate(parts[1:])])
    assert np.array_equal(rp, want[0])
    assert np.array_equal(np.concatenate([p[1] for p in parts]), want[1])
    assert np.array_equal(np.concatenate([p[2] for p in parts]), want[2])


def test_full_size_cage15_rank_slice_refresh(pkg, standins, ctx):
    rows, cols, I, J, V = standins.make("cage15", 1.0)
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    bounds = pkg.split_tile_rows(ctx, A, A, 8)
    lo, hi = int(bounds[0]), int(bounds[1])
    plan = pkg.CPlan(ctx, A, A, lo, hi)
    plan.spgemm()
    V2 = _vals(np.random.default_rng(22), len(I))
    A.set_values(V2[csr_order(I, J)])
    plan.step3()
    got = plan.export_csr()
    plan.close()
    A.close()
    A2 = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V2)
    fresh = pkg.CPlan(ctx, A2, A2, lo, hi)
    fresh.spgemm()
    for x, y in zip(got, fresh.export_csr()):
        assert np.array_equal(x, y)


def test_cache_save_after_refresh_and_refresh_of_loaded(pkg, ctx, tmp_path):
    case = CASES["powerlaw_600"]
    rows, cols, I, J, V, tr = case
    order = csr_order(I, J)
    V2, V3 = _vals(np.random.default_rng(41), len(I)), _vals(np.random.default_rng(42), len(I))
    A, _ = _tilings(pkg, ctx, case, V)
    A.set_values(V2[order])
    path = str(tmp_path / "a.pemt")
    A.save(path)
    L = pkg.Tiled.load(ctx, path)
    want2, _ = _tilings(pkg, ctx, case, V2)
    assert _same(L.array("vals"), want2.array("vals"))
    L.set_values(V3[order])
    want3, _, fresh = _fresh(pkg, ctx, case, V3)
    assert _same(L.array("vals"), want3.array("vals"))
    plan = pkg.CPlan(ctx, L, L)
    plan.spgemm()
    for x, y in zip(_results(plan), _results(fresh)):
        assert _same(x, y)


def test_error_paths(pkg, ctx):
    lib = pkg.lib()
    rows, cols, I, J, V, tr = CASES["rand_50"]
    A = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    F = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V, dtype=np.float32)
    v = np.ascontiguousarray(V)
    f = v.astype(np.float32)
    pv, pf = v.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p)
    for order in (-1, 2):                                                       # bad order
        assert lib.pem_tiled_set_values(ctx._h, A._h, pv, order) == PEM_E_INVALID
    with pytest.raises(ValueError):
        A.set_values(v, order="csc")
    assert lib.pem_tiled_set_values(ctx._h, F._h, pv, 0) == PEM_E_INVALID       # dtype mismatch, both ways and both forms
    assert lib.pem_tiled_set_values_f32(ctx._h, A._h, pf, 0) == PEM_E_INVALID
    assert lib.pem_tiled_set_values_device(ctx._h, F._h, pv, 0) == PEM_E_INVALID
    assert lib.pem_tiled_set_values_device_f32(ctx._h, A._h, pf, 0) == PEM_E_INVALID
    for fn, t in ((lib.pem_tiled_set_values, A), (lib.pem_tiled_set_values_device, A), (lib.pem_tiled_set_values_f32, F),
                  (lib.pem_tiled_set_values_device_f32, F)):                     # null V with nnz > 0
        assert fn(ctx._h, t._h, None, 0) == PEM_E_INVALID
    with pytest.raises(ValueError):
        A.set_values(v[:-1])
    assert _same(A.array("vals"), pkg.Tiled.from_coo(ctx, rows, cols, I, J, V).array("vals"))   # nothing was written
    rows, cols, I, J, V, tr = CASES["empty_matrix"]                                # nnz = 0: a no-op
    E = pkg.Tiled.from_coo(ctx, rows, cols, I, J, V)
    for fn in (lib.pem_tiled_set_values, lib.pem_tiled_set_values_device):
        for order in (0, 1):
            assert fn(ctx._h, E._h, None, order) == 0
    E.set_values(np.zeros(0))
    plan = pkg.CPlan(ctx, E, E)
    plan.spgemm()
    assert plan.info()["nnz_c"] == 0 and len(plan.export_csr()[1]) == 0
