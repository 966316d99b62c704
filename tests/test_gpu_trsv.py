"""GPU: triangular solve on a tiling's lower or upper triangle (pem_tiled_trsv).

Every result is compared with trsvref bit for bit (NaN equal to NaN), in both dtypes and both triangles, and every solve runs down
both routes: narrow levels merged into one launch, and -- by the test hook -- one launch per level.  The cases (trsvcases.py) are
the smallest at which the schedule or the kernel can go wrong: the tile edges, a chain of width-1 levels, two wide levels, wide -
thin - wide, one long row, a random matrix with both triangles stored.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import mxvref as mr
import trsvcases as tc
import trsvref as tr

pytestmark = pytest.mark.gpu

torch.cuda.is_available()   # (torch's runtime first, as in the other GPU files)

CASES = tc.cases()
PEM_E_INVALID = -1
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3.0e-310, 1.0e-40, 0.5, -0.5, 2.0])
IDS = ("f64", "f32")


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


def _rhs(n, seed, dtype):
    return np.random.default_rng(seed).standard_normal(n).astype(dtype)


def _both_routes(ctx, A, b, uplo, unit, want, label):
    """the solve merged and with one launch per level: both equal `want`; returns the two infos"""
    infos = []
    try:
        for split in (False, True):
            ctx.trsv_split(split)
            got = _host(A.trsv(_dev(b), uplo, unit))
            assert _same(got, want), f"{label} {uplo} unit={unit} split={split}: {int(np.sum(got != want))} of {len(want)} differ"
            infos.append(A.trsv_info(uplo))
    finally:
        ctx.trsv_split(False)
    return infos


def _check_case(pkg, ctx, name, dtype, unit=False):
    out = {}
    for side, uplo in enumerate(tr.UPLO):
        n, rp, ci, v = tc.csr(CASES[name][side], dtype)
        A = _tiled(pkg, ctx, n, rp, ci, v, dtype)
        b = _rhs(n, len(name) + side, dtype)
        want = tr.trsv(n, rp, ci, v, b, uplo, unit, dtype)
        merged, split = _both_routes(ctx, A, b, uplo, unit, want, name)
        lv = tr.levels(n, rp, ci, uplo)
        ws = tr.widths(lv)
        for info in (merged, split):
            assert info["levels"] == len(ws) and info["max_width"] == max(ws), (name, uplo, info)
            assert info["missing_diag"] == 0 and info["first_missing_row"] == 0
        assert merged["merge_width"] >= 4 and split["merge_width"] == 0
        assert merged["launches"] == tr.launches(lv, merged["merge_width"]) and split["launches"] == len(ws), (name, uplo, merged, split)
        out[uplo] = (merged, ws)
    return out


# ---- the cases -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", tc.DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ("dense_1", "dense_15", "dense_16", "dense_17", "dense_33"))
def test_tile_edges(pkg, tctx, name, dtype):
    got = _check_case(pkg, tctx, name, dtype)
    for uplo in tr.UPLO:
        assert got[uplo][1] == tc.WIDTHS[name]


@pytest.mark.parametrize("dtype", tc.DTYPES, ids=IDS)
def test_thin_levels_merge_into_one_launch(pkg, tctx, dtype):
    got = _check_case(pkg, tctx, "bidiagonal_200", dtype)
    for uplo in tr.UPLO:
        info, ws = got[uplo]
        assert ws == [1] * 13 and info["launches"] == 1


@pytest.mark.parametrize("dtype", tc.DTYPES, ids=IDS)
def test_wide_levels(pkg, tctx, dtype):
    got = _check_case(pkg, tctx, "grid_40x40_red_black", dtype)
    for uplo in tr.UPLO:
        info, ws = got[uplo]
        assert ws == [50, 50] and info["launches"] == 2


@pytest.mark.parametrize("dtype", tc.DTYPES, ids=IDS)
def test_wide_thin_wide(pkg, tctx, dtype):
    got = _check_case(pkg, tctx, "wide_thin_wide", dtype)
    for uplo in tr.UPLO:
        assert got[uplo][1] == [40, 1, 1, 1, 1, 1, 40]   # (launches against trsvref.launches: _check_case)


@pytest.mark.parametrize("dtype", tc.DTYPES, ids=IDS)
def test_long_row(pkg, tctx, dtype):
    got = _check_case(pkg, tctx, "arrow_400", dtype)
    for uplo in tr.UPLO:
        assert got[uplo][1] == [24, 1]


@pytest.mark.parametrize("dtype", tc.DTYPES, ids=IDS)
def test_random_ignores_the_other_side(pkg, tctx, dtype):
    _check_case(pkg, tctx, "random_600", dtype)
    n, rp, ci, v = tc.csr(CASES["random_600"][0], dtype)
    A = _tiled(pkg, tctx, n, rp, ci, v, dtype)
    b = _dev(_rhs(n, 3, dtype))
    for uplo, op in (("lower", "tril"), ("upper", "triu")):
        T = A.select(op, 0)
        assert 0 < T.nnz < A.nnz
        assert _same(_host(A.trsv(b, uplo)), _host(T.trsv(b, uplo))), uplo


@pytest.mark.parametrize("dtype", tc.DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ("dense_17", "wide_thin_wide", "random_600"))
def test_unit_diagonal(pkg, tctx, name, dtype):
    """stored diagonals set to NaN never reach the result; a tiling without any stored diagonal gives the same bits"""
    for side, uplo in enumerate(tr.UPLO):
        n, I, J, V = CASES[name][side]
        n, rp, ci, v = tc.csr((n, I, J, np.where(I == J, np.nan, V)), dtype)
        b = _rhs(n, 7 + side, dtype)
        want = tr.trsv(n, rp, ci, v, b, uplo, True, dtype)
        assert not np.any(np.isnan(want))
        _both_routes(tctx, _tiled(pkg, tctx, n, rp, ci, v, dtype), b, uplo, True, want, name)
        n, rp, ci, v = tc.csr((n, I, J, V), dtype, drop=I == J)
        if len(v) == 0:
            continue
        B = _tiled(pkg, tctx, n, rp, ci, v, dtype)
        infos = _both_routes(tctx, B, b, uplo, True, want, name + " no diagonal")
        assert infos[0]["missing_diag"] == n and infos[0]["first_missing_row"] == 1


@pytest.mark.parametrize("dtype", tc.DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ("dense_33", "arrow_400", "random_600"))
def test_special_values(pkg, tctx, name, dtype):
    """a quarter of the entries (diagonal included) and of b from +-0, +-inf, NaN and subnormals: what IEEE gives, by bits"""
    for side, uplo in enumerate(tr.UPLO):
        n, I, J, V = CASES[name][side]
        rng = np.random.default_rng(n + side)
        V = V.copy()
        sp = rng.random(len(V)) < 0.25
        V[sp] = rng.choice(SPECIAL, int(sp.sum()))
        n, rp, ci, v = tc.csr((n, I, J, V), dtype)
        b = _rhs(n, 5, dtype)
        sp = rng.random(n) < 0.25
        b[sp] = rng.choice(SPECIAL, int(sp.sum())).astype(dtype)
        want = tr.trsv(n, rp, ci, v, b, uplo, False, dtype)
        assert np.any(np.isnan(want)) and np.any(np.isfinite(want))
        _both_routes(tctx, _tiled(pkg, tctx, n, rp, ci, v, dtype), b, uplo, False, want, name)


# ---- refusals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", tc.DTYPES, ids=IDS)
def test_missing_diagonal(pkg, tctx, dtype):
    n, I, J, V = CASES["random_600"][0]
    n, rp, ci, v = tc.csr((n, I, J, V), dtype, drop=(I == 37) & (J == 37))
    A = _tiled(pkg, tctx, n, rp, ci, v, dtype)
    b = _rhs(n, 1, dtype)
    for uplo in tr.UPLO:
        with pytest.raises(pkg.PemError, match=r"row 38 has no stored diagonal entry") as e:
            A.trsv(_dev(b), uplo)
        assert e.value.status == PEM_E_INVALID
        info = A.trsv_info(uplo)
        assert info["missing_diag"] == 1 and info["first_missing_row"] == 38
        _both_routes(tctx, A, b, uplo, True, tr.trsv(n, rp, ci, v, b, uplo, True, dtype), "row 37 without its diagonal")


def test_other_refusals(pkg, tctx):
    lib = pkg.lib()
    R = pkg.Tiled.from_coo(tctx, 3, 4, [0, 1, 2], [0, 1, 2], [1.0, 1.0, 1.0])
    with pytest.raises(pkg.PemError, match="square"):
        R.trsv(_dev(np.ones(3)))
    with pytest.raises(pkg.PemError, match="square"):
        R.trsv_info()
    n, rp, ci, v = tc.csr(CASES["dense_33"][0])
    A = _tiled(pkg, tctx, n, rp, ci, v, np.float64)
    F = _tiled(pkg, tctx, n, rp, ci, v, np.float32)
    b, x = _dev(np.ones(n)), _dev(np.zeros(n))
    pb, px = C.c_void_p(b.data_ptr()), C.c_void_p(x.data_ptr())
    assert lib.pem_tiled_trsv(tctx._h, F._h, 0, 0, pb, px) == PEM_E_INVALID and b"fp32" in lib.pem_last_error()
    assert lib.pem_tiled_trsv_f32(tctx._h, A._h, 0, 0, pb, px) == PEM_E_INVALID
    for uplo, unit in ((2, 0), (-1, 0), (0, 2), (1, -1)):
        assert lib.pem_tiled_trsv(tctx._h, A._h, uplo, unit, pb, px) == PEM_E_INVALID, (uplo, unit)
    assert lib.pem_tiled_trsv(tctx._h, A._h, 0, 0, None, px) == PEM_E_INVALID
    assert lib.pem_tiled_trsv(tctx._h, A._h, 0, 0, pb, None) == PEM_E_INVALID
    assert lib.pem_tiled_trsv(None, A._h, 0, 0, pb, px) == PEM_E_INVALID
    assert lib.pem_tiled_trsv(tctx._h, None, 0, 0, pb, px) == PEM_E_INVALID
    assert lib.pem_tiled_trsv_info(tctx._h, A._h, 0, None) == PEM_E_INVALID
    buf = _dev(np.ones(n + 8))
    with pytest.raises(pkg.PemError, match="overlap"):
        A.trsv(buf[:n], out=buf[8:])
    with pytest.raises(ValueError, match="uplo"):
        A.trsv(b, "diag")
    with pytest.raises(ValueError, match="uplo"):
        A.trsv_info("full")
    for bad in (np.ones(n), _dev(np.ones(n + 1)), _dev(np.ones(n, np.float32)), _dev(np.ones(2 * n))[::2]):
        with pytest.raises(ValueError):
            A.trsv(bad)
    with pytest.raises(ValueError):
        A.trsv(b, out=_dev(np.ones(n - 1)))
    assert _same(_host(x), np.zeros(n))   # nothing was written by a refused call


def test_empty_shapes(pkg, tctx):
    """an empty tiling: x = b under unit_diag, else every row lacks its diagonal (no binding route makes a 0 x 0 tiling)"""
    E = pkg.Tiled.from_coo(tctx, 40, 40, [], [], [])
    b = _rhs(40, 2, np.float64)
    for uplo in tr.UPLO:
        assert _same(_host(E.trsv(_dev(b), uplo, unit_diag=True)), b)
        with pytest.raises(pkg.PemError, match="row 1 has no stored diagonal"):
            E.trsv(_dev(b), uplo)


# ---- refresh, allocations, in place, the recipe --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", tc.DTYPES, ids=IDS)
def test_refresh_keeps_the_schedule_and_allocates_nothing(pkg, tctx, dtype):
    n, rp, ci, v = tc.csr(CASES["random_600"][0], dtype)
    A = _tiled(pkg, tctx, n, rp, ci, v, dtype)
    b = _rhs(n, 9, dtype)
    db = _dev(b)
    for uplo in tr.UPLO:
        x = torch.empty_like(db)
        A.trsv(db, uplo, out=x)
        assert _same(_host(x), tr.trsv(n, rp, ci, v, b, uplo, False, dtype))
        info = A.trsv_info(uplo)
        v2 = np.where(np.repeat(np.arange(n), np.diff(rp)) == ci, v * dtype(1.5), v[::-1]).astype(dtype)
        A.set_values_device(_dev(v2))
        before = tctx.memory_stats()["block_allocs"]
        A.trsv(db, uplo, out=x)
        x3 = A.trsv(db, uplo, out=db.clone())
        assert tctx.memory_stats()["block_allocs"] == before
        want = tr.trsv(n, rp, ci, v2, b, uplo, False, dtype)
        assert _same(_host(x), want) and _same(_host(x3), want)
        assert A.trsv_info(uplo) == info
        for split in (False, True):   # in place: out is b
            try:
                tctx.trsv_split(split)
                y = db.clone()
                assert A.trsv(y, uplo, out=y) is y
                assert _same(_host(y), want), (uplo, split)
            finally:
                tctx.trsv_split(False)
        A.set_values_device(_dev(v))


@pytest.mark.parametrize("dtype", tc.DTYPES, ids=IDS)
def test_gauss_seidel_recipe(pkg, oracle, tctx, dtype):
    """one forward sweep of section 3x's recipe, (D + L) x' = b - U x, equals mxvref composed with trsvref"""
    n, rp, ci, v = tc.csr(CASES["random_600"][0], dtype)
    A = _tiled(pkg, tctx, n, rp, ci, v, dtype)
    b, x0 = _rhs(n, 21, dtype), _rhs(n, 22, dtype)
    U = A.select("triu", 1)
    db, x = _dev(b), _dev(x0)
    t = torch.empty_like(x)
    U.mxv(x, out=t)
    A.trsv(db - t, "lower", out=x)
    urp, uci, uv = U.export_csr()
    ht = mr.mxv(n, n, urp, uci, uv, x0, "plus_times", dtype, oracle=oracle)
    want = tr.trsv(n, rp, ci, v, (b - ht).astype(dtype), "lower", False, dtype)
    assert _same(_host(x), want)
