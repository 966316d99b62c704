"""GPU: independent sets and aggregation of tilings (pem_tiled_mis / pem_tiled_aggregate).

The central check: A.mis' set, count AND rounds at both distances, and A.aggregate's aggregates, roots, count and rounds, equal
aggref's model exactly -- the sequential greedy set in "beats" order, the two assignment passes -- under the two seeds, all-equal
priorities and test_gpu_colour.py's "ties" array, with the priorities as a host array and as a device int32 tensor, on fp64 and fp32
tilings, with symmetric=False on the pattern as stored and with symmetric=False and symmetric=True on the pattern united with its
transpose.  The references are computed once per (graph, priorities) and never changed."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import aggref as ar
import colourref as cr
from matgen import cases

pytestmark = pytest.mark.gpu

torch.cuda.is_available()   # (torch's runtime first, as in the other GPU files)

CASES = cases()
PEM_E_INVALID = -1
DTYPES = (np.float64, np.float32)
GRAPHS = ar.graphs(CASES)
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
    """None for a seed (hashed in registers), else the uint32 array"""
    return None if which in SEEDS else ar.priority_array(n, which)


@functools.lru_cache(maxsize=None)
def _model(name, which):
    """((in_set, count, rounds) at distance 1, the same at distance 2, (agg, roots, naggregates, rounds)) of the model; never changed"""
    n, I, J = GRAPHS[name]
    prio = ar.priority_array(n, which)
    out = (ar.mis(n, I, J, 1, priority=prio), ar.mis(n, I, J, 2, priority=prio), ar.aggregate(n, I, J, priority=prio))
    for res in out:
        for a in res[:2]:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return out


def _tiled(pkg, ctx, n, I, J, dtype, seed=1):
    V = np.random.default_rng(seed).standard_normal(len(I))
    return pkg.Tiled.from_coo(ctx, n, n, I, J, V, dtype=dtype)


def _args(n, which, device_priority):
    p = _priority(n, which)
    if p is not None and device_priority:
        p = _dev(p.view(np.int32))                    # an int32 tensor is read as uint32
    return dict(seed=which if which in SEEDS else 99, priority=p)


def _mis(A, n, distance, which, symmetric, device_priority=False):
    s, count, rounds = A.mis(distance=distance, symmetric=symmetric, **_args(n, which, device_priority))
    assert s.dtype == torch.uint8 and s.is_cuda and s.numel() == n
    return _host(s), count, rounds


def _aggregate(A, n, which, symmetric, device_priority=False):
    agg, roots, nc, rounds = A.aggregate(symmetric=symmetric, **_args(n, which, device_priority))
    assert agg.dtype == roots.dtype == torch.int32 and agg.is_cuda and roots.is_cuda and agg.numel() == n and roots.numel() == nc
    return _host(agg), _host(roots), nc, rounds


def _same(got, want):
    return all(np.array_equal(g, w) if isinstance(w, np.ndarray) else g == w for g, w in zip(got, want)) and len(got) == len(want)


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_sets_aggregates_and_rounds_equal_the_model(pkg, tctx, name):
    n, I, J = GRAPHS[name]
    Is, Js = cr.symmetrised(I, J) if len(I) else (I, J)
    for k, dtype in enumerate(DTYPES):
        A = _tiled(pkg, tctx, n, I, J, dtype)
        S = _tiled(pkg, tctx, n, Is, Js, dtype)
        for which in PRIORITIES:
            want = _model(name, which)
            for distance in (1, 2):
                got = _mis(A, n, distance, which, False, device_priority=bool(k))
                assert _same(got, want[distance - 1]), (name, which, distance, dtype.__name__, got[1:], want[distance - 1][1:])
                on_s = _mis(S, n, distance, which, False)
                promised = _mis(S, n, distance, which, True, device_priority=not k)
                assert _same(on_s, want[distance - 1]), (name, which, distance, "symmetrised")
                assert _same(promised, on_s), (name, which, distance, "symmetric=True")
            got = _aggregate(A, n, which, False, device_priority=bool(k))
            assert _same(got, want[2]), (name, which, dtype.__name__, got[2:], want[2][2:])
            on_s = _aggregate(S, n, which, False)
            promised = _aggregate(S, n, which, True, device_priority=not k)
            assert _same(on_s, want[2]), (name, which, "symmetrised")
            assert _same(promised, on_s), (name, which, "symmetric=True")
        A.close()
        S.close()


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_the_distance_1_set_is_colour_0(pkg, tctx, name):
    """the colouring's kernel is independent of these: its colour 0 is the greedy maximal independent set"""
    n, I, J = GRAPHS[name]
    A = _tiled(pkg, tctx, n, I, J, np.float64)
    for which in PRIORITIES:
        kw = _args(n, which, False)
        s, count, _ = A.mis(distance=1, **kw)
        c, _, _ = A.colour(**kw)
        assert torch.equal(s, (c == 0).to(torch.uint8)) and count == int((c == 0).sum()), (name, which)
    A.close()


def test_the_figures_the_graphs_pin_down(pkg, tctx):
    """what the issue states for single graphs, read off the device"""
    def run(name, which):
        n, I, J = GRAPHS[name]
        A = _tiled(pkg, tctx, n, I, J, np.float64)
        agg, _, nc, rounds = _aggregate(A, n, which, False)
        return _mis(A, n, 1, which, False)[1:], (nc, rounds), int(np.bincount(agg).max())
    for name in ("empty_matrix", "one_entry", "diag_100"):
        n = GRAPHS[name][0]
        assert run(name, 0) == ((n, 1), (n, 1), 1) and run(name, "ties") == ((n, 1), (n, 1), 1)
    for name in ("dense_tile", "dense_48", "k131"):
        assert run(name, 12345) == ((1, 2), (1, 2), GRAPHS[name][0]) and run(name, "equal") == ((1, 2), (1, 2), GRAPHS[name][0])
    assert run("k70_in_75", 0) == ((6, 2), (6, 2), 70)
    assert run("hub_row_4000", 0) == ((1842, 7), (1, 2), 4000) and run("hub_row_4000", 12345) == ((1819, 8), (1, 2), 4000)
    assert run("band_1500", 0) == ((205, 11), (17, 6), 119) and run("band_1500", "equal") == ((222, 58), (22, 42), 159)
    assert run("path_203_one_way", 12345) == ((87, 6), (59, 4), 5)
    assert run("path_203_one_way", "equal") == ((102, 203), (68, 136), 3)          # the column direction counts; n rounds
    assert run("powerlaw_600", 0) == ((225, 8), (41, 12), 137) and run("rand_300", 12345) == ((60, 7), (14, 10), 39)
    assert run("empty_rows", 0) == ((101, 4), (62, 6), 12)
    assert run("grid_40_one_way", 0) == ((594, 7), (233, 10), 11) and run("grid_40_one_way", "equal") == ((800, 79), (280, 85), 7)


def test_a_false_symmetry_promise_still_ends_in_bounds(pkg, tctx):
    """symmetric=True on a pattern stored one way: PEM_OK, every in_set byte 0 or 1, every agg in [-1, naggregates)"""
    n, I, J = GRAPHS["path_203_one_way"]
    A = _tiled(pkg, tctx, n, I, J, np.float64)
    for which in PRIORITIES:
        for distance in (1, 2):
            s, count, rounds = _mis(A, n, distance, which, True)
            assert set(np.unique(s)) <= {0, 1}
        agg, roots, nc, rounds = _aggregate(A, n, which, True)
        assert agg.min() >= -1 and agg.max() < nc


def test_galerkin_coarse_operator_equals_scipy(pkg, tctx):
    """one coarsening level by INTEGRATION.md's recipe: Ac = P^T (A P) with integer values, so every sum is exact"""
    sp = pytest.importorskip("scipy.sparse", reason="the Galerkin reference is scipy's P.T @ A @ P")
    for name in ("rand_300", "band_1500", "grid_40_one_way"):
        n, I, J = GRAPHS[name]
        V = np.random.default_rng(11).integers(1, 4, len(I)) * np.random.default_rng(12).choice([-1, 1], len(I))
        A = pkg.Tiled.from_coo(tctx, n, n, I, J, V.astype(np.float64))
        agg, roots, nc, _ = A.aggregate()
        P = pkg.prolongator(tctx, agg, nc)
        assert (P.rows, P.cols, P.nnz) == (n, nc, n)
        Pt = P.transpose()
        ap = pkg.CPlan(tctx, A, P)
        ap.spgemm()
        AP = pkg.Tiled.from_cplan(ap)
        g = pkg.CPlan(tctx, Pt, AP)
        g.spgemm()
        Ac = pkg.Tiled.from_cplan(g)
        rp, ci, v = Ac.export_csr()
        want_agg = _model(name, 0)[2]
        assert np.array_equal(_host(agg), want_agg[0]) and nc == want_agg[2]
        Ph = sp.csr_matrix((np.ones(n), (np.arange(n), want_agg[0])), shape=(n, nc))
        Ah = sp.csr_matrix((V.astype(np.float64), (I, J)), shape=(n, n))
        want = (Ph.T.tocsr() @ Ah @ Ph).tocsr()
        want.eliminate_zeros()   # scipy's product drops the sums that cancel to 0 (some versions; all of them after this)
        want.sort_indices()
        assert (Ac.rows, Ac.cols) == (nc, nc)
        # the device keeps a product's structural pattern, cancelled sums included as stored zeros: the pattern of |P|^T |A| |P|,
        # where nothing cancels, with P^T A P's values on it ...
        struct = (Ph.T.tocsr() @ abs(Ah) @ Ph).tocsr()
        struct.sort_indices()
        assert struct.data.min() > 0
        dense = want.toarray()
        srows = np.repeat(np.arange(nc), np.diff(struct.indptr))
        assert np.array_equal(rp, struct.indptr) and np.array_equal(ci, struct.indices) and np.array_equal(v, dense[srows, struct.indices]), name
        # ... and, the stored zeros dropped (section 3g's select), scipy's P.T @ A @ P array for array
        rp, ci, v = Ac.select("value_ne", 0).export_csr()
        assert np.array_equal(rp, want.indptr) and np.array_equal(ci, want.indices) and np.array_equal(v, want.data), name
    # a near-null-space vector as the values, and the refusal of a vertex without an aggregate
    vals = torch.arange(1, n + 1, dtype=torch.float32, device="cuda")
    P32 = pkg.prolongator(tctx, agg, nc, values=vals, dtype=np.float32)
    rp, ci, v = P32.export_csr()
    assert np.array_equal(rp, np.arange(n + 1)) and np.array_equal(ci, want_agg[0]) and np.array_equal(v, np.arange(1, n + 1, dtype=np.float32))
    bad = agg.clone()
    bad[7] = -1
    with pytest.raises(ValueError, match="outside"):
        pkg.prolongator(tctx, bad, nc)
    with pytest.raises(ValueError, match="outside"):
        pkg.prolongator(tctx, agg, nc - 1)
    with pytest.raises(ValueError, match="values"):
        pkg.prolongator(tctx, agg, nc, values=vals)            # float32 values for a float64 prolongator


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_explicit_zeros_and_nans_are_edges(pkg, tctx, dtype):
    n = 40
    I = np.array([3, 33, 7, 8, 20, 21], np.int32)
    J = np.array([20, 5, 8, 7, 21, 20], np.int32)
    V = np.array([0.0, np.nan, 1.0, -0.0, 2.0, np.inf])
    A = pkg.Tiled.from_coo(tctx, n, n, I, J, V, dtype=dtype)
    for which in PRIORITIES:
        kw = dict(seed=which if which in SEEDS else 0, priority=_priority(n, which))
        for distance in (1, 2):
            s, count, rounds = A.mis(distance=distance, **kw)
            s = _host(s)
            assert _same((s, count, rounds), ar.mis(n, I, J, distance, **kw))
            assert s[3] + s[20] <= 1 and s[33] + s[5] == 1 and s[7] + s[8] == 1   # the zero's edge, the NaN's edge, the -0's edge
        agg, roots, nc, rounds = A.aggregate(**kw)
        assert _same((_host(agg), _host(roots), nc, rounds), ar.aggregate(n, I, J, **kw))
        agg = _host(agg)
        assert agg[33] == agg[5] and agg[7] == agg[8] and agg[3] == agg[20] == agg[21]


def test_outs_are_written_in_place_and_two_calls_are_identical(pkg, tctx):
    n, I, J = GRAPHS["powerlaw_600"]
    A = _tiled(pkg, tctx, n, I, J, np.float64)
    out_s = torch.full((n,), 77, dtype=torch.uint8, device="cuda")
    out_a = torch.full((n,), POISON, dtype=torch.int32, device="cuda")
    for which in PRIORITIES:
        p = _priority(n, which)
        seed = which if which in SEEDS else 0
        for symmetric in (False, True):
            for distance in (2, 1):
                s1, c1, r1 = A.mis(distance=distance, seed=seed, priority=p, symmetric=symmetric, out=out_s)
                assert s1 is out_s
                first = _host(out_s).tobytes()
                tctx.synchronize()
                before = tctx.memory_stats()
                s2, c2, r2 = A.mis(distance=distance, seed=seed, priority=None if p is None else _dev(p.view(np.int32)), symmetric=symmetric)
                after = tctx.memory_stats()
                assert _host(s2).tobytes() == first and (c1, r1) == (c2, r2), (which, symmetric, distance)
                for key in ("block_allocs", "driver_allocs", "slab_bytes", "in_use_bytes"):
                    assert after[key] == before[key], f"mis {which} symmetric={symmetric}: a repeat call changed {key}"
            a1, roots1, n1, r1 = A.aggregate(seed=seed, priority=p, symmetric=symmetric, out=out_a)
            assert a1 is out_a
            first, first_roots = _host(out_a).tobytes(), _host(roots1).tobytes()
            tctx.synchronize()
            before = tctx.memory_stats()
            a2, roots2, n2, r2 = A.aggregate(seed=seed, priority=p, symmetric=symmetric)
            nothing = A.aggregate(seed=seed, priority=p, symmetric=symmetric, roots=False)
            after = tctx.memory_stats()
            assert _host(a2).tobytes() == first and _host(roots2).tobytes() == first_roots and (n1, r1) == (n2, r2), (which, symmetric)
            assert nothing[1] is None and _host(nothing[0]).tobytes() == first and nothing[2:] == (n1, r1)
            for key in ("block_allocs", "driver_allocs", "slab_bytes", "in_use_bytes"):
                assert after[key] == before[key], f"aggregate {which} symmetric={symmetric}: a repeat call changed {key}"
    # a smaller graph on the same context allocates nothing either
    m, I2, J2 = GRAPHS["ragged_37"]
    B = _tiled(pkg, tctx, m, I2, J2, np.float64)
    B.aggregate()
    B.mis()
    before = tctx.memory_stats()["block_allocs"]
    B.aggregate(seed=5)
    B.mis(seed=5, distance=1)
    assert tctx.memory_stats()["block_allocs"] == before
    with pytest.raises(ValueError, match="uint8"):
        A.mis(out=torch.zeros(n, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="uint8"):
        A.mis(out=torch.zeros(n + 1, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="int32"):
        A.aggregate(out=torch.zeros(n, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="priority"):
        A.mis(priority=torch.zeros(n, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="priority"):
        A.aggregate(priority=np.zeros(n - 1, np.uint32))
    with pytest.raises(ValueError, match="seed"):
        A.aggregate(seed=-1)
    for distance in (0, 3, True, 1.5, None):
        with pytest.raises(ValueError, match="distance"):
            A.mis(distance=distance)


def test_invalid_arguments_leave_the_outputs_untouched(pkg, tctx):
    L = pkg.lib()
    n, I, J = GRAPHS["ragged_37"]
    A = _tiled(pkg, tctx, n, I, J, np.float64)
    rows, cols, RI, RJ, RV, _ = CASES["rect_33x65_AAt"]
    R = pkg.Tiled.from_coo(tctx, rows, cols, RI, RJ, RV)
    big = max(n, rows, cols)
    in_set = torch.full((16 * big,), 77, dtype=torch.uint8, device="cuda")
    agg = torch.full((big,), POISON, dtype=torch.int32, device="cuda")
    root = torch.full((big,), POISON, dtype=torch.int32, device="cuda")
    count, rounds = C.c_int64(POISON), C.c_int32(POISON)
    P = lambda t, off=0: None if t is None else C.c_void_p(t.data_ptr() + off)

    def mis(ctx=tctx._h, a=A._h, d=2, sym=0, dp=None, ds=P(in_set), pn=C.byref(count), pr=C.byref(rounds)):
        return L.pem_tiled_mis(ctx, a, d, sym, 0, dp, ds, pn, pr)

    def aggregate(ctx=tctx._h, a=A._h, sym=0, dp=None, da=P(agg), dr=P(root), pn=C.byref(count), pr=C.byref(rounds)):
        return L.pem_tiled_aggregate(ctx, a, sym, 0, dp, da, dr, pn, pr)

    tctx.synchronize()
    before = tctx.memory_stats()
    bad = [mis(ctx=None), mis(a=None), mis(ds=None), mis(pn=None), mis(pr=None),
           mis(a=R._h), mis(a=R._h, sym=1),                                      # 33 x 65
           mis(d=0), mis(d=3), mis(d=-1), mis(sym=2), mis(sym=-1),
           mis(dp=P(in_set)),                                                    # the priorities ARE the set
           mis(dp=P(in_set, n - 1)),                                             # the last byte of the set is the first of the priorities
           mis(dp=P(in_set, 4 * n), ds=P(in_set, 8 * n - 1)),                    # the first byte of the set is the last of the priorities
           aggregate(ctx=None), aggregate(a=None), aggregate(da=None), aggregate(pn=None), aggregate(pr=None),
           aggregate(a=R._h), aggregate(sym=2), aggregate(sym=-1),
           aggregate(dp=P(agg)), aggregate(dp=P(agg, 4 * (n - 1))), aggregate(dp=P(agg, -4 * (n - 1))),
           aggregate(dp=P(root)), aggregate(dp=P(root, 4 * (n - 1))),
           aggregate(dr=P(agg)), aggregate(dr=P(agg, 4 * (n - 1))), aggregate(dr=P(agg, -4 * (n - 1)))]
    assert bad == [PEM_E_INVALID] * len(bad)
    assert tctx.memory_stats() == before, "a refused call touched the context's memory"
    assert np.all(_host(in_set) == 77) and np.all(_host(agg) == POISON) and np.all(_host(root) == POISON)
    assert (count.value, rounds.value) == (POISON, POISON)
    # what is legal next to them: adjacent buffers, and no d_root
    both = torch.zeros(3 * n, dtype=torch.int32, device="cuda")
    assert aggregate(dp=P(both), da=P(both, 4 * n), dr=P(both, 8 * n)) == 0
    want = ar.aggregate(n, I, J, priority=np.zeros(n, np.uint32))
    got = _host(both)
    assert np.array_equal(got[n:2 * n], want[0]) and (count.value, rounds.value) == want[2:] and np.all(got[:n] == 0)
    assert np.array_equal(got[2 * n:2 * n + want[2]], want[1]) and np.all(got[2 * n + want[2]:] == -1)   # d_root: the roots, then -1
    assert aggregate(dr=None) == 0 and np.all(_host(root) == POISON)
    with pytest.raises(pkg.PemError):
        R.mis()
    with pytest.raises(pkg.PemError):
        R.aggregate()


def test_the_empty_tiling(pkg, tctx):
    """n = 0 is not constructible as a tiling (the library's (0, 0) for it is reached by no binding route; the model's is in
    test_aggregate_cpu.py); the empty tiling: every vertex in the set and an aggregate of its own, one round"""
    n, I, J = GRAPHS["empty_matrix"]
    assert len(I) == 0
    for dtype in DTYPES:
        A = _tiled(pkg, tctx, n, I, J, dtype)
        for symmetric in (False, True):
            for distance in (1, 2):
                s, count, rounds = _mis(A, n, distance, 0, symmetric)
                assert np.all(s == 1) and (count, rounds) == (n, 1)
            agg, roots, nc, rounds = _aggregate(A, n, 12345, symmetric)
            assert np.array_equal(agg, np.arange(n)) and np.array_equal(roots, np.arange(n)) and (nc, rounds) == (n, 1)
