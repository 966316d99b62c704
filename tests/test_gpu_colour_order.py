"""GPU: the colour order (pem_colour_order) and the reordering built on it.

colour_order equals numpy's stable argsort by colour and the cumulative histogram -- on colourings the device made, on a random
colour array of 100 003 vertices, for n = 0 and for one colour; a colour outside [0, ncolours) is refused after the call's wait.
End to end: R, p, off = A.reorder_by_colour() is the host reindexing of A by p (extractref), R's lower schedule has no more levels
than A's (strictly fewer on the band), and trsv and ilu0 on R match their references (trsvref, ilu0ref)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import colourref as cr
import extractref as ex
import ilu0ref as ir
import trsvcases as tc
import trsvref as tr
from matgen import cases

pytestmark = pytest.mark.gpu

torch.cuda.is_available()

CASES = cases()
PEM_E_INVALID = -1
GRAPHS = {name: (CASES[name][0], CASES[name][2], CASES[name][3]) for name in ("ragged_37", "hub_row_4000", "band_1500", "empty_matrix")}
GRAPHS.update(cr.built_graphs())


@pytest.fixture(scope="module")
def tctx(pkg):
    """a context on a torch stream made current for the module (see test_gpu_mxv.py)"""
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


def _check_order(pkg, ctx, colours, ncolours):
    perm, off = pkg.colour_order(ctx, _dev(colours), ncolours)
    assert perm.dtype == torch.int32 and off.dtype == torch.int32 and perm.is_cuda and off.is_cuda
    wp, wo = cr.colour_order(colours, ncolours)
    assert np.array_equal(_host(perm), np.argsort(colours, kind="stable").astype(np.int32)) and np.array_equal(_host(perm), wp)
    assert np.array_equal(_host(off), wo) and len(wo) == ncolours + 1


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_order_of_device_colourings(pkg, tctx, name):
    n, I, J = GRAPHS[name]
    A = pkg.Tiled.from_coo(tctx, n, n, I, J, np.ones(len(I)))
    for seed, prio in ((0, None), (12345, None), (0, np.zeros(n, np.uint32))):
        c, nc, _ = A.colour(seed=seed, priority=prio)
        perm, off = pkg.colour_order(tctx, c, nc)
        ch = _host(c)
        wp, wo = cr.colour_order(ch, nc)
        assert np.array_equal(_host(perm), wp) and np.array_equal(_host(off), wo), (name, seed)


def test_order_of_given_colours(pkg, tctx):
    rng = np.random.default_rng(11)
    _check_order(pkg, tctx, rng.integers(0, 7, 100_003).astype(np.int32), 7)
    _check_order(pkg, tctx, rng.integers(0, 7, 100_003).astype(np.int32), 9)        # two colours nobody holds
    _check_order(pkg, tctx, rng.integers(0, 1000, 5_000).astype(np.int32), 1000)    # more than one sort digit
    _check_order(pkg, tctx, np.zeros(777, np.int32), 1)                              # one colour
    _check_order(pkg, tctx, np.zeros(1, np.int32), 1)
    _check_order(pkg, tctx, np.zeros(0, np.int32), 0)                                # n = 0
    _check_order(pkg, tctx, np.zeros(0, np.int32), 3)
    _check_order(pkg, tctx, np.arange(300, dtype=np.int32)[::-1].copy(), 300)        # every vertex its own colour, reversed
    # two calls give the same bytes, and the second allocates nothing
    c = _dev(rng.integers(0, 5, 4097).astype(np.int32))
    p1, o1 = pkg.colour_order(tctx, c, 5)
    tctx.synchronize()
    before = tctx.memory_stats()["block_allocs"]
    p2, o2 = pkg.colour_order(tctx, c, 5)
    assert tctx.memory_stats()["block_allocs"] == before
    assert _host(p1).tobytes() == _host(p2).tobytes() and _host(o1).tobytes() == _host(o2).tobytes()


def test_a_colour_out_of_range_is_refused(pkg, tctx):
    base = np.random.default_rng(3).integers(0, 4, 1000).astype(np.int32)
    for bad in (4, -1, 2 ** 31 - 1, -2 ** 31):
        c = base.copy()
        c[613] = bad
        with pytest.raises(pkg.PemError) as e:
            pkg.colour_order(tctx, _dev(c), 4)
        assert e.value.status == PEM_E_INVALID and "outside" in str(e.value)
    _check_order(pkg, tctx, base, 4)   # the context works on


def test_invalid_arguments(pkg, tctx):
    L = pkg.lib()
    n, k = 100, 3
    colour = _dev(np.random.default_rng(1).integers(0, k, n).astype(np.int32))
    perm = torch.full((n,), -5, dtype=torch.int32, device="cuda")
    off = torch.full((k + 1,), -5, dtype=torch.int32, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())

    def call(ctx=tctx._h, nn=n, dc=P(colour), kk=k, dp=P(perm), do=P(off)):
        return L.pem_colour_order(ctx, C.c_int64(nn), dc, C.c_int32(kk), dp, do)

    tctx.synchronize()
    before = tctx.memory_stats()
    buf = torch.zeros(3 * n, dtype=torch.int32, device="cuda")
    b0 = buf.data_ptr()
    bad = [call(ctx=None), call(dc=None), call(dp=None), call(do=None), call(nn=-1), call(nn=2 ** 31), call(kk=-1), call(kk=0),
           call(dc=C.c_void_p(b0), dp=C.c_void_p(b0 + 4 * (n - 1))),            # colours and perm
           call(dc=C.c_void_p(b0), do=C.c_void_p(b0 + 4 * (n - 1))),            # colours and offsets
           call(dp=C.c_void_p(b0), do=C.c_void_p(b0 + 4 * (n - 1))),            # perm and offsets
           call(dp=C.c_void_p(b0 + 4 * k), do=C.c_void_p(b0))]                  # the last offset is the first of perm
    assert bad == [PEM_E_INVALID] * len(bad)
    assert tctx.memory_stats() == before, "a refused call touched the context's memory"
    assert np.all(_host(perm) == -5) and np.all(_host(off) == -5)
    assert call(dp=C.c_void_p(b0 + 4 * (k + 1)), do=C.c_void_p(b0)) == 0         # adjacent is legal
    wp, wo = cr.colour_order(_host(colour), k)
    assert np.array_equal(_host(buf)[:k + 1], wo) and np.array_equal(_host(buf)[k + 1:k + 1 + n], wp)
    with pytest.raises(ValueError, match="ncolours"):
        pkg.colour_order(tctx, colour, -1)
    with pytest.raises(ValueError, match="ncolours = 0"):
        pkg.colour_order(tctx, colour, 0)
    with pytest.raises(ValueError, match="int32 tensor"):
        pkg.colour_order(tctx, colour.to(torch.int64), k)


# ---- end to end: the reordering and what it is for ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _problem(name):
    """the graph with standard normal values and a dominant diagonal (trsvcases): (n, I, J, V), never changed"""
    n, _, I, J, _, _ = CASES[name]
    off = I != J
    return tc._finish(n, I[off], J[off], np.random.default_rng(len(name)))


@pytest.mark.parametrize("name", ("powerlaw_600", "band_1500"))
def test_reorder_by_colour_end_to_end(pkg, tctx, name):
    n, I, J, V = _problem(name)
    A = pkg.Tiled.from_coo(tctx, n, n, I, J, V)
    R, p, off = A.reorder_by_colour()
    c, nc, _ = A.colour()
    ph = _host(p)
    wp, wo = cr.colour_order(_host(c), nc)
    assert np.array_equal(ph, wp) and np.array_equal(_host(off), wo) and sorted(ph) == list(range(n))
    model = cr.colouring(n, I, J, seed=0)
    assert np.array_equal(_host(c), model[0]) and nc == model[1]
    # R is the host reindexing of A by p
    ni, nj, RI, RJ, RV = ex.extract(n, n, I, J, V, ph, ph)
    case = (n, RI.astype(np.int64), RJ.astype(np.int64), RV)
    _, rp, ci, v = tc.csr(case)
    grp, gci, gv = R.export_csr()
    assert (R.rows, R.cols, R.nnz) == (n, n, len(V))
    assert np.array_equal(grp, rp) and np.array_equal(gci, ci) and _same(gv, v)
    # inside a colour no vertex has a neighbour: the diagonal blocks of R are diagonal
    oh = _host(off)
    block = np.searchsorted(oh, RI, "right")
    assert np.all((block != np.searchsorted(oh, RJ, "right")) | (RI == RJ))
    for uplo in tr.UPLO:
        la, lr = A.trsv_info(uplo)["levels"], R.trsv_info(uplo)["levels"]
        assert lr == len(tr.widths(tr.levels(n, rp, ci, uplo)))
        assert lr <= la and (name != "band_1500" or lr < la), (name, uplo, la, lr)
        b = np.random.default_rng(7).standard_normal(n)
        assert _same(_host(R.trsv(_dev(b), uplo)), tr.trsv(n, rp, ci, v, b, uplo, False, np.float64)), (name, uplo)
    f, _ = ir.ilu0(n, rp, ci, v, np.float64)
    F = R.ilu0()
    frp, fci, fv = F.export_csr()
    assert np.array_equal(frp, rp) and np.array_equal(fci, ci) and _same(fv, f)
    # R keeps its provenance: new values of A reach it through the extract's refresh
    A.set_values(np.asarray(tc.csr((n, I, J, 2.0 * V))[3]))
    R.set_values_from_extract(A)
    assert _same(R.export_csr()[2], 2.0 * v)
    # the promise of a symmetric pattern, on one: the same reordering
    Is, Js = cr.symmetrised(I, J)
    S = pkg.Tiled.from_coo(tctx, n, n, Is, Js, np.ones(len(Is)))
    R1, p1, o1 = S.reorder_by_colour(seed=12345, symmetric=True)
    R0, p0, o0 = S.reorder_by_colour(seed=12345, symmetric=False)
    assert np.array_equal(_host(p1), _host(p0)) and np.array_equal(_host(o1), _host(o0))
    assert np.array_equal(R1.export_csr()[1], R0.export_csr()[1])
