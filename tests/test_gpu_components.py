"""GPU: connected components of tilings (pem_tiled_components).

The central check: A.components' labels, ids, ncomponents AND rounds equal ccref's model exactly -- the rounds of the contract in
numpy -- and the labels equal scipy's, on fp64 and fp32 tilings, with symmetric=False on the pattern as stored and with
symmetric=True on the pattern united with its transpose, which must equal symmetric=False on that same tiling.  The references are
computed once per graph and never changed."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import ccref as cc
from matgen import cases

pytestmark = pytest.mark.gpu

torch.cuda.is_available()   # (torch's runtime first, as in the other GPU files)

CASES = cases()
PEM_E_INVALID = -1
DTYPES = (np.float64, np.float32)
NAMES = ("one_entry", "empty_matrix", "diag_100", "tiny_9x9", "rand_50", "ragged_37", "dense_tile", "dense_48", "empty_rows", "rand_300",
         "powerlaw_600", "hub_row_4000", "band_1500")
GRAPHS = {name: (CASES[name][0], CASES[name][2], CASES[name][3]) for name in NAMES}
GRAPHS.update(cc.built_graphs())
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


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _model(name):
    """(labels, ids, ncomponents, rounds) of the model, the labels checked against scipy; never changed"""
    n, I, J = GRAPHS[name]
    labels, rounds = cc.components_model(n, I, J)
    assert np.array_equal(labels, cc.components_scipy(n, I, J))
    ids, nc = cc.ids_of(labels)
    labels.setflags(write=False)
    ids.setflags(write=False)
    return labels, ids, nc, rounds


def _tiled(pkg, ctx, n, I, J, dtype, seed=1):
    V = np.random.default_rng(seed).standard_normal(len(I))
    return pkg.Tiled.from_coo(ctx, n, n, I, J, V, dtype=dtype)


def _components(A, n, symmetric, **kw):
    labels, ids, nc, rounds = A.components(symmetric=symmetric, **kw)
    assert labels.dtype == torch.int32 and labels.is_cuda and labels.numel() == n
    assert ids is None or (ids.dtype == torch.int32 and ids.is_cuda and ids.numel() == n)
    return _host(labels), None if ids is None else _host(ids), nc, rounds


def _equal(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and tuple(got[2:]) == tuple(want[2:])


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_labels_ids_count_and_rounds_equal_the_model(pkg, tctx, name):
    n, I, J = GRAPHS[name]
    want = _model(name)
    Is, Js = cc.symmetrised(I, J) if len(I) else (I, J)
    for dtype in DTYPES:
        A = _tiled(pkg, tctx, n, I, J, dtype)
        S = _tiled(pkg, tctx, n, Is, Js, dtype)
        got = _components(A, n, False)
        assert _equal(got, want), (name, dtype.__name__, got[2:], want[2:])
        on_s = _components(S, n, False)
        promised = _components(S, n, True)
        assert _equal(on_s, want), (name, dtype.__name__, "symmetrised", on_s[2:], want[2:])
        assert _equal(promised, on_s), (name, dtype.__name__, "symmetric=True", promised[2:], on_s[2:])
        A.close()
        S.close()


def test_the_figures_the_graphs_pin_down(pkg, tctx):
    """(components, rounds) the contract states for single graphs, read off the device"""
    def run(name):
        n, I, J = GRAPHS[name]
        A = _tiled(pkg, tctx, n, I, J, np.float64)
        return _components(A, n, False)[2:]
    assert run("one_entry") == (5, 1) and run("empty_matrix") == (40, 1) and run("diag_100") == (100, 1)   # no off-diagonal entry: 1 round
    assert run("dense_tile") == (1, 2) and run("dense_48") == (1, 2) and run("k131") == (1, 2)              # several chunks per line
    assert run("k70_in_75") == (6, 2) and run("empty_rows") == (25, 5) and run("hub_row_4000") == (1, 3)
    # stored one way: the column orientation must be walked
    assert run("path_203_one_way") == (1, 9) and run("path_4097_down") == (1, 14) and run("star_in_2000") == (2, 3)


@pytest.mark.parametrize("name", ("ragged_37", "k70_in_75"))
def test_nothing_is_written_past_a_partial_last_line(pkg, tctx, name):
    n, I, J = GRAPHS[name]
    assert n % 16
    want = _model(name)
    A = _tiled(pkg, tctx, n, I, J, np.float64)
    big_l = torch.full((n + 64,), POISON, dtype=torch.int32, device="cuda")
    big_i = torch.full((n + 64,), POISON, dtype=torch.int32, device="cuda")
    for symmetric in (False, True):
        labels, ids, nc, rounds = A.components(symmetric=symmetric, out=big_l[:n], out_ids=big_i[:n])
        assert labels.data_ptr() == big_l.data_ptr() and ids.data_ptr() == big_i.data_ptr()
        assert np.all(_host(big_l)[n:] == POISON) and np.all(_host(big_i)[n:] == POISON)
        if not symmetric or name == "k70_in_75":   # (k70's pattern is symmetric)
            assert _equal((_host(big_l)[:n], _host(big_i)[:n], nc, rounds), want)


def test_two_calls_are_identical_and_allocate_nothing(pkg, tctx):
    n, I, J = GRAPHS["grid_64_shuffled"]
    A = _tiled(pkg, tctx, n, I, J, np.float64)
    out = torch.full((n,), POISON, dtype=torch.int32, device="cuda")
    out_ids = torch.full((n,), POISON, dtype=torch.int32, device="cuda")
    for symmetric in (False, True):
        l1, i1, nc1, r1 = A.components(symmetric=symmetric, out=out, out_ids=out_ids)
        assert l1 is out and i1 is out_ids
        first = _host(out).tobytes(), _host(out_ids).tobytes()
        tctx.synchronize()
        before = tctx.memory_stats()
        l2, i2, nc2, r2 = A.components(symmetric=symmetric)
        after = tctx.memory_stats()
        assert (_host(l2).tobytes(), _host(i2).tobytes()) == first and (nc1, r1) == (nc2, r2), symmetric
        for key in ("block_allocs", "driver_allocs", "slab_bytes", "in_use_bytes"):
            assert after[key] == before[key], f"symmetric={symmetric}: a repeat call changed {key}"
    # a smaller graph after a larger one on the same context: correct, no stale label leaks, nothing allocated
    for name in ("empty_rows", "ragged_37", "sparse_forest_3000"):
        m, I2, J2 = GRAPHS[name]
        B = _tiled(pkg, tctx, m, I2, J2, np.float64)
        B.components()   # (builds B's column schedule)
        before = tctx.memory_stats()["block_allocs"]
        got = _components(B, m, False)
        assert tctx.memory_stats()["block_allocs"] == before
        assert _equal(got, _model(name)), name
    with pytest.raises(ValueError, match="int32"):
        A.components(out=torch.zeros(n, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="int32"):
        A.components(out_ids=torch.zeros(n + 1, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="ids=False"):
        A.components(ids=False, out_ids=out_ids)


def test_without_ids(pkg, tctx):
    for name in ("sparse_forest_3000", "two_cycles_1025"):
        n, I, J = GRAPHS[name]
        want = _model(name)
        A = _tiled(pkg, tctx, n, I, J, np.float32)
        labels, ids, nc, rounds = _components(A, n, False, ids=False)
        assert ids is None and np.array_equal(labels, want[0]) and (nc, rounds) == want[2:]


def test_explicit_zeros_nans_and_diagonals(pkg, tctx):
    n = 40
    I = np.array([3, 33, 7, 8, 20, 21, 9, 11], np.int32)
    J = np.array([20, 5, 8, 7, 21, 20, 9, 11], np.int32)
    V = np.array([0.0, np.nan, 1.0, -0.0, 2.0, np.inf, 0.0, 3.0])
    labels, rounds = cc.components_model(n, I, J)
    assert np.array_equal(labels, cc.components_scipy(n, I, J))
    for dtype in DTYPES:
        A = pkg.Tiled.from_coo(tctx, n, n, I, J, V, dtype=dtype)
        got = _components(A, n, False)
        assert _equal(got, (labels,) + cc.ids_of(labels) + (rounds,))
        assert got[0][20] == 3 and got[0][21] == 3 and got[0][33] == 5 and got[0][8] == 7 and got[0][9] == 9 and got[0][11] == 11


def test_derived_tilings(pkg, tctx):
    """a tiling from a plan, a select and a transpose label like the tiling converted from their export"""
    n, _, I, J, V, _ = CASES["rand_300"]
    A = pkg.Tiled.from_coo(tctx, n, n, I, J, V)
    plan = pkg.CPlan(tctx, A, A)
    plan.spgemm()
    for T in (pkg.Tiled.from_cplan(plan), A.select("triu", 1), A.select("triu", 1).transpose(), A.select("row_le", 120)):
        rp, ci, v = T.export_csr()
        ri = np.repeat(np.arange(n, dtype=np.int32), np.diff(rp))
        E = pkg.Tiled.from_coo(tctx, n, n, ri, ci, v)
        labels, rounds = cc.components_model(n, ri, ci)
        want = (labels,) + cc.ids_of(labels) + (rounds,)
        assert np.array_equal(labels, cc.components_scipy(n, ri, ci))
        assert _equal(_components(T, n, False), want) and _equal(_components(E, n, False), want)


def test_a_false_symmetry_promise_still_ends_in_bounds(pkg, tctx):
    """symmetric=True on a pattern stored one way: the values are unspecified, but 0 <= label[v] <= v and the call ends"""
    n, I, J = GRAPHS["path_203_one_way"]
    A = _tiled(pkg, tctx, n, I, J, np.float64)
    labels, ids, nc, rounds = _components(A, n, True)
    assert np.all(labels >= 0) and np.all(labels <= np.arange(n))


@pytest.mark.parametrize("name", ("empty_rows", "sparse_forest_3000"))
def test_reorder_by_component(pkg, tctx, name):
    n, I, J = GRAPHS[name]
    V = np.random.default_rng(9).standard_normal(len(I))
    A = pkg.Tiled.from_coo(tctx, n, n, I, J, V)
    R, perm, offsets = A.reorder_by_component()
    labels, ids, nc, _ = _model(name)
    ph, oh = _host(perm), _host(offsets)
    assert np.array_equal(ph, np.argsort(ids, kind="stable").astype(np.int32))
    assert np.array_equal(oh, np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=nc))]).astype(np.int32)) and len(oh) == nc + 1
    # blocks in order of smallest vertex, vertices ascending inside a block
    assert np.array_equal(ph[oh[:-1]], np.flatnonzero(labels == np.arange(n))) and all(np.all(np.diff(ph[oh[c]:oh[c + 1]]) > 0) for c in range(nc))
    rp, ci, v = R.export_csr()
    ri = np.repeat(np.arange(n), np.diff(rp))
    assert np.array_equal(np.searchsorted(oh, ri, "right"), np.searchsorted(oh, ci, "right"))   # block diagonal
    W = sp.coo_matrix((V, (I, J)), shape=(n, n)).tocsr()[ph][:, ph].tocsr()
    W.sort_indices()
    assert (R.rows, R.cols, R.nnz) == (n, n, len(V))
    assert np.array_equal(rp, W.indptr) and np.array_equal(ci, W.indices) and v.tobytes() == W.data.tobytes()
    # block c, cut out of R and out of A, is the same matrix
    c = int(np.argmax(np.diff(oh)))
    lo, hi = int(oh[c]), int(oh[c + 1])
    B1, B2 = R.extract(slice(lo, hi), slice(lo, hi)), A.extract(perm[lo:hi], perm[lo:hi])
    e1, e2 = B1.export_csr(), B2.export_csr()
    assert B1.rows == hi - lo and all(np.array_equal(x, y) for x, y in zip(e1, e2))
    assert np.array_equal(e1[0], W[lo:hi][:, lo:hi].indptr)
    # R keeps its provenance
    W2 = sp.coo_matrix((2.0 * V, (I, J)), shape=(n, n)).tocsr()
    W2.sort_indices()
    A.set_values(np.asarray(W2.data))
    R.set_values_from_extract(A)
    assert R.export_csr()[2].tobytes() == (2.0 * W.data).tobytes()
    # the promise, on a symmetric pattern: the same reordering
    Is, Js = cc.symmetrised(I, J)
    S = pkg.Tiled.from_coo(tctx, n, n, Is, Js, np.ones(len(Is)))
    _, p1, o1 = S.reorder_by_component(symmetric=True)
    assert np.array_equal(_host(p1), ph) and np.array_equal(_host(o1), oh)


def test_invalid_arguments_leave_the_outputs_untouched(pkg, tctx):
    L = pkg.lib()
    n, I, J = GRAPHS["ragged_37"]
    A = _tiled(pkg, tctx, n, I, J, np.float64)
    rows, cols, RI, RJ, RV, _ = CASES["rect_33x65_AAt"]
    R = pkg.Tiled.from_coo(tctx, rows, cols, RI, RJ, RV)
    big = max(n, rows, cols)
    buf = torch.full((3 * big,), POISON, dtype=torch.int32, device="cuda")
    b0 = buf.data_ptr()
    nc, rounds = C.c_int64(POISON), C.c_int32(POISON)
    P = C.c_void_p

    def call(ctx=tctx._h, a=A._h, sym=0, dl=P(b0), di=P(b0 + 4 * big), pn=C.byref(nc), pr=C.byref(rounds)):
        return L.pem_tiled_components(ctx, a, sym, dl, di, pn, pr)

    tctx.synchronize()
    before = tctx.memory_stats()
    bad = [call(ctx=None), call(a=None), call(dl=None), call(pn=None), call(pr=None), call(dl=None, di=None),
           call(a=R._h), call(a=R._h, sym=1),                                   # 33 x 65
           call(sym=2), call(sym=-1),
           call(di=P(b0)),                                                      # the ids ARE the labels
           call(di=P(b0 + 4 * (n - 1))),                                        # the last label is the first id
           call(dl=P(b0 + 4 * big), di=P(b0 + 4 * big - 4 * (n - 1)))]
    assert bad == [PEM_E_INVALID] * len(bad)
    assert tctx.memory_stats() == before, "a refused call touched the context's memory"
    assert np.all(_host(buf) == POISON) and (nc.value, rounds.value) == (POISON, POISON)
    # what is legal next to them: adjacent buffers, and no ids
    want = _model("ragged_37")
    assert call(di=P(b0 + 4 * n)) == 0
    h = _host(buf)
    assert _equal((h[:n], h[n:2 * n], nc.value, rounds.value), want) and np.all(h[2 * n:] == POISON)
    assert call(dl=P(b0 + 4 * 2 * big), di=None) == 0
    assert np.array_equal(_host(buf)[2 * big:2 * big + n], want[0]) and (nc.value, rounds.value) == want[2:]
    with pytest.raises(pkg.PemError):
        R.components()


def test_the_empty_tiling(pkg, tctx):
    """n = 0 is not constructible as a tiling; the empty tiling: every vertex its own component, one round"""
    n, I, J = GRAPHS["empty_matrix"]
    assert len(I) == 0
    for dtype in DTYPES:
        A = _tiled(pkg, tctx, n, I, J, dtype)
        for symmetric in (False, True):
            labels, ids, nc, rounds = _components(A, n, symmetric)
            assert (nc, rounds) == (40, 1) and np.array_equal(labels, np.arange(40)) and np.array_equal(ids, np.arange(40))
