"""GPU: graph colouring of tilings (pem_tiled_colour).

The central check: A.colour's colours, ncolours AND rounds equal colourref's model exactly -- the sequential greedy colouring in
descending (priority, -index) order, whose rounds are the longest chain of falling priority -- under the two seeds, under all-equal
priorities (tools/trsv_pass.py's natural-order colouring) and under a random priority array drawn with many ties, on fp64 and fp32
tilings, with symmetric=False on the pattern as stored and with symmetric=True on the pattern united with its transpose, which must
equal symmetric=False on that same tiling.  The references are computed once per (graph, priorities) and never changed."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import colourref as cr
from matgen import cases

pytestmark = pytest.mark.gpu

torch.cuda.is_available()   # (torch's runtime first, as in the other GPU files)

CASES = cases()
PEM_E_INVALID = -1
DTYPES = (np.float64, np.float32)
NAMES = ("one_entry", "empty_matrix", "diag_100", "ragged_37", "dense_tile", "dense_48", "empty_rows", "rand_300", "powerlaw_600",
         "hub_row_4000", "band_1500")
GRAPHS = {name: (CASES[name][0], CASES[name][2], CASES[name][3]) for name in NAMES}
GRAPHS.update(cr.built_graphs())
SEEDS = (0, 12345)
PRIORITIES = SEEDS + ("equal", "ties")
POISON = -77777


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


def _priority(n, which):
    """None for a seed (hashed in registers), else the uint32 array: all equal, or four values so that most neighbours tie"""
    if which in SEEDS:
        return None
    if which == "equal":
        return np.full(n, 0x80000000, np.uint32)
    return np.random.default_rng(n + 5).integers(0, 4, n).astype(np.uint32) * np.uint32(0x40000001)


@functools.lru_cache(maxsize=None)
def _model(name, which):
    """(colours, ncolours, rounds) of the model; never changed"""
    n, I, J = GRAPHS[name]
    seed = which if which in SEEDS else 0
    c, nc, rounds = cr.colouring(n, I, J, seed=seed, priority=_priority(n, which))
    assert cr.is_valid(n, I, J, c)
    c.setflags(write=False)
    return c, nc, rounds


def _tiled(pkg, ctx, n, I, J, dtype, seed=1):
    V = np.random.default_rng(seed).standard_normal(len(I))
    return pkg.Tiled.from_coo(ctx, n, n, I, J, V, dtype=dtype)


def _colour(A, n, which, symmetric, device_priority=False):
    p = _priority(n, which)
    if p is not None and device_priority:
        p = _dev(p.view(np.int32))                    # an int32 tensor is read as uint32
    c, nc, rounds = A.colour(seed=which if which in SEEDS else 99, priority=p, symmetric=symmetric)
    assert c.dtype == torch.int32 and c.is_cuda and c.numel() == n
    return _host(c), nc, rounds


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_colours_and_rounds_equal_the_model(pkg, tctx, name):
    n, I, J = GRAPHS[name]
    Is, Js = cr.symmetrised(I, J) if len(I) else (I, J)
    for k, dtype in enumerate(DTYPES):
        A = _tiled(pkg, tctx, n, I, J, dtype)
        S = _tiled(pkg, tctx, n, Is, Js, dtype)
        for which in PRIORITIES:
            want = _model(name, which)
            got = _colour(A, n, which, False, device_priority=bool(k))
            assert np.array_equal(got[0], want[0]) and got[1:] == want[1:], (name, which, dtype.__name__, got[1:], want[1:])
            on_s = _colour(S, n, which, False)
            promised = _colour(S, n, which, True, device_priority=not k)
            assert np.array_equal(on_s[0], want[0]) and on_s[1:] == want[1:], (name, which, "symmetrised")
            assert np.array_equal(promised[0], on_s[0]) and promised[1:] == on_s[1:], (name, which, "symmetric=True")
        A.close()
        S.close()


def test_the_figures_the_graphs_pin_down(pkg, tctx):
    """what the issue states for single graphs, read off the device"""
    def run(name, which):
        n, I, J = GRAPHS[name]
        A = _tiled(pkg, tctx, n, I, J, np.float64)
        return _colour(A, n, which, False)
    assert run("one_entry", 0)[1:] == (1, 1) and run("empty_matrix", 0)[1:] == (1, 1) and run("diag_100", 0)[1:] == (1, 1)
    assert run("dense_tile", 0)[1:] == (16, 16) and run("dense_48", 12345)[1:] == (48, 48)
    assert run("hub_row_4000", 0)[1:] == (6, 14) and run("hub_row_4000", 12345)[1:] == (6, 16)
    assert run("band_1500", "equal")[2] == 270
    c, nc, rounds = run("k70_in_75", 0)
    assert (nc, rounds) == (70, 70) and np.all(c[70:] == 0) and sorted(c[:70]) == list(range(70))   # one window overflow
    assert run("k131", 12345)[1:] == (131, 131)                                                     # two window advances
    assert run("path_203_one_way", "equal")[1:] == (2, 203)                                         # the column direction counts
    assert run("path_203_one_way", 0)[1:] == (3, 5) and run("path_203_one_way", 12345)[1:] == (3, 6)


def test_a_false_symmetry_promise_still_ends_in_bounds(pkg, tctx):
    """symmetric=True on a pattern stored one way: the colours are unspecified, but every one is in [0, n) and the call ends"""
    for name in ("path_203_one_way", "rand_300", "hub_row_4000"):
        n, I, J = GRAPHS[name]
        A = _tiled(pkg, tctx, n, I, J, np.float64)
        for which in PRIORITIES:
            c, nc, rounds = _colour(A, n, which, True)
            assert c.min() >= 0 and c.max() < n and nc == c.max() + 1 and 1 <= rounds <= n
            # (unspecified by the contract, but determined: the rounds on what the row orientation alone sees.  The sequential greedy
            # order does not describe them here -- a vertex may see a neighbour of lower priority that did not wait for it)
            prio = cr.hash_priority(n, which) if which in SEEDS else _priority(n, which)
            wc, _, wnc, wrounds = cr.jones_plassmann(cr.adjacency(n, I, J, symmetric=True), prio)
            assert np.array_equal(c, wc) and (nc, rounds) == (wnc, wrounds), (name, which)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_explicit_zeros_and_nans_are_edges(pkg, tctx, dtype):
    n = 40
    I = np.array([3, 33, 7, 8, 20, 21], np.int32)
    J = np.array([20, 5, 8, 7, 21, 20], np.int32)
    V = np.array([0.0, np.nan, 1.0, -0.0, 2.0, np.inf])
    A = pkg.Tiled.from_coo(tctx, n, n, I, J, V, dtype=dtype)
    for which in PRIORITIES:
        c, nc, rounds = A.colour(seed=which if which in SEEDS else 0, priority=_priority(n, which))
        c = _host(c)
        want = cr.colouring(n, I, J, seed=which if which in SEEDS else 0, priority=_priority(n, which))
        assert np.array_equal(c, want[0]) and (nc, rounds) == want[1:]
        assert c[3] != c[20] and c[33] != c[5] and c[7] != c[8]   # the zero's edge, the NaN's edge, the -0's edge


def test_out_is_written_in_place_and_two_calls_are_identical(pkg, tctx):
    n, I, J = GRAPHS["powerlaw_600"]
    A = _tiled(pkg, tctx, n, I, J, np.float64)
    out = torch.full((n,), POISON, dtype=torch.int32, device="cuda")
    for which in PRIORITIES:
        p = _priority(n, which)
        seed = which if which in SEEDS else 0
        for symmetric in (False, True):
            c1, nc1, r1 = A.colour(seed=seed, priority=p, symmetric=symmetric, out=out)
            assert c1 is out
            first = _host(out).tobytes()
            tctx.synchronize()
            before = tctx.memory_stats()
            c2, nc2, r2 = A.colour(seed=seed, priority=None if p is None else _dev(p.view(np.int32)), symmetric=symmetric)
            after = tctx.memory_stats()
            assert _host(c2).tobytes() == first and (nc1, r1) == (nc2, r2), (which, symmetric)
            for key in ("block_allocs", "driver_allocs", "slab_bytes", "in_use_bytes"):
                assert after[key] == before[key], f"{which} symmetric={symmetric}: a repeat call changed {key}"
    # a smaller graph on the same context allocates nothing either
    m, I2, J2 = GRAPHS["ragged_37"]
    B = _tiled(pkg, tctx, m, I2, J2, np.float64)
    B.colour(symmetric=False)
    before = tctx.memory_stats()["block_allocs"]
    B.colour(seed=5, symmetric=False)
    assert tctx.memory_stats()["block_allocs"] == before
    with pytest.raises(ValueError, match="int32"):
        A.colour(out=torch.zeros(n, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="int32"):
        A.colour(out=torch.zeros(n + 1, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="priority"):
        A.colour(priority=torch.zeros(n, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="priority"):
        A.colour(priority=torch.zeros(n - 1, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="priority"):
        A.colour(priority=np.zeros(n - 1, np.uint32))
    with pytest.raises(ValueError, match="seed"):
        A.colour(seed=-1)


def test_invalid_arguments_leave_the_colours_untouched(pkg, tctx):
    L = pkg.lib()
    n, I, J = GRAPHS["ragged_37"]
    A = _tiled(pkg, tctx, n, I, J, np.float64)
    rows, cols, RI, RJ, RV, _ = CASES["rect_33x65_AAt"]
    R = pkg.Tiled.from_coo(tctx, rows, cols, RI, RJ, RV)
    big = max(n, rows, cols)
    colour = torch.full((big,), POISON, dtype=torch.int32, device="cuda")
    prio = torch.zeros(big, dtype=torch.int32, device="cuda")
    nc, rounds = C.c_int32(POISON), C.c_int32(POISON)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def call(ctx=tctx._h, a=A._h, sym=0, seed=0, dp=None, dc=P(colour), pn=C.byref(nc), pr=C.byref(rounds)):
        return L.pem_tiled_colour(ctx, a, sym, C.c_uint32(seed), dp, dc, pn, pr)

    tctx.synchronize()
    before = tctx.memory_stats()
    bad = [call(ctx=None), call(a=None), call(dc=None), call(pn=None), call(pr=None),
           call(a=R._h), call(a=R._h, sym=1),                                   # 33 x 65
           call(sym=2), call(sym=-1),
           call(dp=P(colour)),                                                  # the priorities ARE the colours
           call(dp=C.c_void_p(colour.data_ptr() + 4 * (n - 1))),                # the last colour is the first priority
           call(dp=C.c_void_p(colour.data_ptr() - 4 * (n - 1)))]
    assert bad == [PEM_E_INVALID] * len(bad)
    assert tctx.memory_stats() == before, "a refused call touched the context's memory"
    assert np.all(_host(colour) == POISON) and (nc.value, rounds.value) == (POISON, POISON)
    # what is legal next to them: adjacent buffers
    both = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    assert call(dp=C.c_void_p(both.data_ptr()), dc=C.c_void_p(both.data_ptr() + 4 * n)) == 0
    want = cr.colouring(n, I, J, priority=np.zeros(n, np.uint32))
    assert np.array_equal(_host(both)[n:], want[0]) and (nc.value, rounds.value) == want[1:] and np.all(_host(both)[:n] == 0)
    with pytest.raises(pkg.PemError):
        R.colour()
