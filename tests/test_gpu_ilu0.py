"""GPU: ILU(0) of a tiling on its own pattern (pem_tiled_ilu0).

Every factor is compared with ilu0ref bit for bit (NaN equal to NaN), in both dtypes and down both launch routes: narrow levels merged
into one launch, and -- by the test hook -- one launch per level.  The cases (ilu0cases.py) are the smallest at which the schedule or
the kernel can go wrong.  The references are computed once per (case, dtype) and shared.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ilu0cases as ic
import ilu0ref as ir
import trsvref as tr

pytestmark = pytest.mark.gpu

torch.cuda.is_available()   # (torch's runtime first, as in the other GPU files)

CASES = ic.cases()
PEM_E_INVALID = -1
IDS = ("f64", "f32")
ARRAYS = ("tile_keys", "tile_nnz_ptr", "masks", "rowptr", "rowcolidx", "vals", "masks_t", "tile_rowptr", "tile_colidx", "tile_colptr",
          "tile_rowidx", "tile_offsets")
INFO = ("rows", "cols", "nnz", "tile_rows", "tile_cols", "ntiles", "value_bytes")


@pytest.fixture(scope="module")
def tctx(pkg):
    """a context on a torch stream made current for the module: torch's work and the library's calls are ordered with no extra sync"""
    prev = torch.cuda.current_stream()
    s = torch.cuda.Stream()
    torch.cuda.set_stream(s)
    c = pkg.Context(0, stream=s.cuda_stream)
    yield c
    c.close()
    torch.cuda.set_stream(prev)


@functools.lru_cache(maxsize=None)
def _ref(name, dtype):
    """(n, rp, ci, a, f, levels): the case as CSR, its reference factor and the levels of its lower schedule; never changed"""
    n, rp, ci, a = ic.csr(CASES[name], dtype)
    f, _ = ir.ilu0(n, rp, ci, a, dtype)
    return n, rp, ci, a, f, tr.levels(n, rp, ci, "lower")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    return bool(np.all((got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want))))


def _tiled(pkg, ctx, n, rp, ci, v, dtype):
    I = np.repeat(np.arange(n, dtype=np.int32), np.diff(rp))
    return pkg.Tiled.from_coo(ctx, n, n, I, np.asarray(ci, np.int32), v, dtype=dtype)


def _same_tiling(got, want):
    """the pattern and every pem_tiled_info / array field but the build times"""
    for k in INFO:
        assert getattr(got, k) == getattr(want, k), k
    for name in ARRAYS:
        g, w = got.array(name), want.array(name)
        assert _same(g, w) if name == "vals" else np.array_equal(g, w), name


def _routes(ctx):
    for split in (False, True):
        ctx.trsv_split(split)
        yield split


# ---- the cases -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ic.DTYPES, ids=IDS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_factor_matches_the_reference(pkg, tctx, name, dtype):
    n, rp, ci, a, f, lv = _ref(name, dtype)
    ws = tr.widths(lv)
    if name in ic.WIDTHS:
        assert ws == ic.WIDTHS[name]
    A = _tiled(pkg, tctx, n, rp, ci, a, dtype)
    want = _tiled(pkg, tctx, n, rp, ci, f, dtype)
    b = np.random.default_rng(len(name)).standard_normal(n).astype(dtype)
    t = tr.trsv(n, rp, ci, f, b, "lower", True, dtype)
    z = tr.trsv(n, rp, ci, f, t, "upper", False, dtype)
    frp, fci, fv = want.transpose().export_csr()
    try:
        for split in _routes(tctx):
            F = A.ilu0()
            grp, gci, gv = F.export_csr()
            assert np.array_equal(grp, rp) and np.array_equal(gci, ci)
            assert _same(gv, f), f"{name} split={split}: {int(np.sum(gv != f))} of {len(f)} values differ"
            _same_tiling(F, want)
            info = F.ilu0_info()
            assert info["levels"] == len(ws) and info["max_width"] == max(ws), (name, info)
            assert info["zero_pivots"] == 0 and info["first_zero_pivot_row"] == 0
            if split:
                assert info["merge_width"] == 0 and info["launches"] == len(ws), info
            else:
                assert info["merge_width"] >= 4 and info["launches"] == tr.launches(lv, info["merge_width"]), info
            # the preconditioner solve, by hand and by lu_solve
            db = _dev(b)
            work = torch.empty_like(db)
            F.trsv(db, "lower", unit_diag=True, out=work)
            assert _same(_host(work), t)
            assert _same(_host(F.trsv(work, "upper")), z)
            assert _same(_host(F.lu_solve(db)), z) and _same(_host(F.lu_solve(db, out=torch.empty_like(db), work=work)), z)
            # vals_t: the transpose reads the column-major copy
            trp, tci, tv = F.transpose().export_csr()
            assert np.array_equal(trp, frp) and np.array_equal(tci, fci) and _same(tv, fv)
    finally:
        tctx.trsv_split(False)


def test_thin_levels_merge_and_wide_levels_do_not(pkg, tctx):
    for name, merged_launches in (("tridiagonal_200", 1), ("grid_40x40_red_black", 2), ("wide_thin_wide", 3)):
        n, rp, ci, a, f, lv = _ref(name, np.float64)
        F = _tiled(pkg, tctx, n, rp, ci, a, np.float64).ilu0()
        assert F.ilu0_info()["launches"] == merged_launches, name


@pytest.mark.parametrize("dtype", ic.DTYPES, ids=IDS)
def test_factor_is_an_ordinary_tiling(pkg, tctx, tmp_path, dtype):
    """mxv, save / load and a plan's operand all read the factor like any tiling"""
    n, rp, ci, a, f, _ = _ref("random_300", dtype)
    F = _tiled(pkg, tctx, n, rp, ci, a, dtype).ilu0()
    want = _tiled(pkg, tctx, n, rp, ci, f, dtype)
    x = _dev(np.random.default_rng(8).standard_normal(n).astype(dtype))
    assert _same(_host(F.mxv(x)), _host(want.mxv(x)))
    assert _same(_host(F.mxv(x, transpose=True)), _host(want.mxv(x, transpose=True)))
    path = str(tmp_path / "f.pemtile")
    F.save(path)
    _same_tiling(pkg.Tiled.load(tctx, path), want)
    pf, pw = pkg.CPlan(tctx, F, F), pkg.CPlan(tctx, want, want)
    pf.spgemm()
    pw.spgemm()
    for g, w in zip(pf.export_csr(), pw.export_csr()):
        assert _same(g, w) if g.dtype.kind == "f" else np.array_equal(g, w)


# ---- refresh ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ic.DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ("random_300", "wide_thin_wide"))
def test_refresh_equals_a_fresh_factor(pkg, tctx, name, dtype):
    n, rp, ci, a, f, _ = _ref(name, dtype)
    A = _tiled(pkg, tctx, n, rp, ci, a, dtype)
    diag = np.repeat(np.arange(n), np.diff(rp)) == ci
    a2 = np.where(diag, a * dtype(1.5), a[::-1]).astype(dtype)
    b = np.random.default_rng(3).standard_normal(n).astype(dtype)
    db = _dev(b)
    try:
        for split in _routes(tctx):
            A.set_values(a)
            F = A.ilu0()
            z0 = _host(F.lu_solve(db))   # (builds both of F's trsv schedules)
            infos = F.trsv_info("lower"), F.trsv_info("upper")
            A.set_values(a2)
            before = tctx.memory_stats()["block_allocs"]
            F.set_values_from_ilu0(A)
            assert tctx.memory_stats()["block_allocs"] == before   # the refresh allocates nothing
            fresh = A.ilu0()
            assert _same(F.array("vals"), fresh.array("vals")) and _same(F.export_csr()[2], fresh.export_csr()[2]), (name, split)
            assert _same(F.transpose().export_csr()[2], fresh.transpose().export_csr()[2])
            assert (F.trsv_info("lower"), F.trsv_info("upper")) == infos   # the schedules survive
            z = _host(F.lu_solve(db))
            assert _same(z, _host(fresh.lu_solve(db))) and not _same(z, z0)   # the solve uses the new values
    finally:
        tctx.trsv_split(False)
    f2, _ = ir.ilu0(n, rp, ci, a2, dtype)
    assert _same(F.export_csr()[2], f2)


# ---- special values --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ic.DTYPES, ids=IDS)
def test_special_values(pkg, tctx, dtype):
    tiny = 1.0e-40 if dtype is np.float32 else 3.0e-310   # subnormal in the dtype
    probes = {
        # a zero pivot: f_10 = 3 / 0 = inf, f_11 = fma(-inf, 2, 4) = -inf ... what IEEE gives
        "zero pivot": (2, [0, 2, 4], [0, 1, 0, 1], [0.0, 2.0, 3.0, 4.0], 2, 1),
        # 0 / 0: NaN below the pivot, NaN from there on
        "zero over zero": (2, [0, 2, 4], [0, 1, 0, 1], [0.0, 2.0, 0.0, 4.0], 2, 1),
        "subnormals": (3, [0, 3, 6, 9], [0, 1, 2] * 3, [tiny, tiny * 3, 1.0, tiny * 5, 2.0, tiny, 0.5, tiny, tiny * 7], None, None),
        # a_00 = 0, (1, 0) and (1, 1) stored, (0, 1) not stored: f_11 = a_11, not NaN
        "unstored is not zero": (3, [0, 1, 3, 4], [0, 0, 1, 2], [0.0, 1.0, 5.0, 2.0], 1, 1),
    }
    try:
        for split in _routes(tctx):
            for label, (n, rp, ci, v, zp, first) in probes.items():
                rp, ci, v = np.array(rp, np.int64), np.array(ci, np.int64), np.array(v, dtype)
                f, _ = ir.ilu0(n, rp, ci, v, dtype)
                F = _tiled(pkg, tctx, n, rp, ci, v, dtype).ilu0()
                got = F.export_csr()[2]
                assert _same(got, f), (label, split, got, f)
                info = F.ilu0_info()
                if zp is not None:
                    assert info["zero_pivots"] == zp and info["first_zero_pivot_row"] == first, (label, info)
                else:
                    d = f[ci == np.repeat(np.arange(n), np.diff(rp))]
                    bad = ~np.isfinite(d) | (d == 0)
                    assert info["zero_pivots"] == int(bad.sum()), (label, info)
                if label == "unstored is not zero":
                    assert np.isinf(got[1]) and got[2] == dtype(5.0)
                if label == "zero pivot":
                    assert np.isinf(got[2]) and not np.isfinite(got[3])
    finally:
        tctx.trsv_split(False)


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_nothing_behind(pkg, tctx):
    lib = pkg.lib()
    n, rp, ci, a, f, _ = _ref("random_300", np.float64)
    A = _tiled(pkg, tctx, n, rp, ci, a, np.float64)
    A.ilu0().close()   # (the arena has served one factor: a refused call must leave its use where it was)
    in_use = tctx.memory_stats()["in_use_bytes"]
    R = pkg.Tiled.from_coo(tctx, 3, 4, [0, 1, 2], [0, 1, 2], [1.0, 1.0, 1.0])
    with pytest.raises(pkg.PemError, match="square") as e:
        R.ilu0()
    assert e.value.status == PEM_E_INVALID
    with pytest.raises(pkg.PemError, match="square"):
        R.ilu0_info()
    R.close()
    drop = (np.repeat(np.arange(n), np.diff(rp)) == 37) & (ci == 37)
    I = np.repeat(np.arange(n, dtype=np.int32), np.diff(rp))
    M = pkg.Tiled.from_coo(tctx, n, n, I[~drop], ci[~drop].astype(np.int32), a[~drop])
    with pytest.raises(pkg.PemError, match=r"pem_tiled_ilu0: row 38 has no stored diagonal entry") as e:
        M.ilu0()
    assert e.value.status == PEM_E_INVALID
    M.close()
    E = pkg.Tiled.from_coo(tctx, 40, 40, [], [], [])   # (no binding route makes a 0 x 0 tiling: the empty one is n = 40)
    with pytest.raises(pkg.PemError, match="row 1 has no stored diagonal"):
        E.ilu0()
    E.close()
    assert tctx.memory_stats()["in_use_bytes"] == in_use
    F = A.ilu0()
    B = _tiled(pkg, tctx, n, rp, ci, a, np.float64)
    before = F.array("vals")
    with pytest.raises(pkg.PemError, match="not made by pem_tiled_ilu0 from this A"):
        F.set_values_from_ilu0(B)   # another tiling, even of the same pattern
    with pytest.raises(pkg.PemError, match="not made by pem_tiled_ilu0 from this A"):
        B.set_values_from_ilu0(A)   # a tiling not made by ilu0
    with pytest.raises(pkg.PemError, match="not made by pem_tiled_ilu0 from this A"):
        A.apply("abs").set_values_from_ilu0(A)
    assert _same(F.array("vals"), before)
    h = C.c_void_p(0xdead)
    assert lib.pem_tiled_ilu0(None, A._h, C.byref(h)) == PEM_E_INVALID and h.value is None
    h = C.c_void_p(0xdead)
    assert lib.pem_tiled_ilu0(tctx._h, None, C.byref(h)) == PEM_E_INVALID and h.value is None
    assert lib.pem_tiled_ilu0(tctx._h, A._h, None) == PEM_E_INVALID
    for args in ((None, F._h, A._h), (tctx._h, None, A._h), (tctx._h, F._h, None)):
        assert lib.pem_tiled_set_values_from_ilu0(*args) == PEM_E_INVALID
    info = pkg.Ilu0Info()
    for args in ((None, F._h, C.byref(info)), (tctx._h, None, C.byref(info)), (tctx._h, F._h, None)):
        assert lib.pem_tiled_ilu0_info(*args) == PEM_E_INVALID
    assert _same(F.array("vals"), before)
