"""Host model of the connected components (pem_tiled_components), written from the contract: the rounds
the device runs -- grandparents, the neighbours' minimum, the hooks onto the vertex and onto its parent, all taken on one snapshot --
in numpy, scipy's components mapped to smallest-vertex labels, the dense ids, and the graphs the tests build themselves."""
import numpy as np

from colourref import built_graphs as _colour_graphs
from colourref import symmetrised  # noqa: F401  (the tests take it from here)

NONE = np.iinfo(np.int64).max


def components_model(n, I, J, symmetric_walk=False):
    """(labels, rounds): the rounds of the contract.  The state is f, started at f[v] = v.  A round: gp = f[f]; m[v] = the minimum of
    gp[u] over v's neighbours u; f'[x] = min(gp[x], m[x], min{m[v] : f[v] == x}); the call ends after the first round with f' == f,
    that round counted.  symmetric_walk=False unites the entries with their transposes (both orientations are walked);
    symmetric_walk=True reads the row orientation only: vertex i sees j for a stored (i, j)."""
    I, J = np.asarray(I, np.int64), np.asarray(J, np.int64)
    near, far = (I, J) if symmetric_walk else (np.concatenate([I, J]), np.concatenate([J, I]))
    f = np.arange(n, dtype=np.int64)
    rounds = 0
    while True:
        rounds += 1
        gp = f[f]
        m = np.full(n, NONE, np.int64)
        np.minimum.at(m, near, gp[far])
        fn = np.minimum(gp, m)
        np.minimum.at(fn, f, m)
        if np.array_equal(fn, f) or rounds >= max(n, 1):
            return fn.astype(np.int32), rounds
        f = fn


def components_scipy(n, I, J):
    """labels by scipy: connected_components(directed=False), every scipy label mapped to the smallest vertex of its component"""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    I, J = np.asarray(I, np.int64), np.asarray(J, np.int64)
    A = sp.coo_matrix((np.ones(len(I), np.int8), (I, J)), shape=(n, n)).tocsr()
    nc, lab = connected_components(A, directed=False)
    smallest = np.full(nc, n, np.int64)
    np.minimum.at(smallest, lab, np.arange(n))
    return smallest[lab].astype(np.int32)


def ids_of(labels):
    """(ids, ncomponents): the dense ids 0 .. ncomponents - 1 in order of smallest vertex -- ids[v] = the number of roots below
    labels[v]"""
    labels = np.asarray(labels, np.int64)
    root = labels == np.arange(len(labels))
    rank = np.cumsum(root) - root
    return rank[labels].astype(np.int32), int(root.sum())


def _random_entries(n, count, seed):
    """about `count` distinct random entries of an n x n pattern, sorted"""
    g = np.random.default_rng(seed)
    key = np.unique(g.integers(0, n, count).astype(np.int64) * n + g.integers(0, n, count))
    return (key // n).astype(np.int32), (key % n).astype(np.int32)


def built_graphs():
    """name -> (n, I, J): colourref's three graphs and the seven built for the components, all seeded"""
    out = dict(_colour_graphs())
    i32 = lambda a: np.asarray(a, np.int32)
    p = np.arange(4096)
    out["path_4097_down"] = (4097, i32(p + 1), i32(p))                                   # (i + 1, i): the column direction hooks
    q = np.random.default_rng(5000).permutation(5000)
    out["path_5000_shuffled"] = (5000, i32(q[:-1]), i32(q[1:]))
    q = np.random.default_rng(64).permutation(64 * 64).reshape(64, 64)                    # a 64 x 64 grid, every edge stored one way
    out["grid_64_shuffled"] = (4096, i32(np.concatenate([q[:, :-1].ravel(), q[:-1, :].ravel()])),
                               i32(np.concatenate([q[:, 1:].ravel(), q[1:, :].ravel()])))
    out["sparse_forest_3000"] = (3000,) + _random_entries(3000, 1200, 3000)
    out["star_in_2000"] = (2000, i32(np.arange(1, 2000)), i32(np.full(1999, 1999)))       # vertex 0 stays alone
    q = np.random.default_rng(1025).permutation(1025)
    a, b = q[:500], q[500:]
    out["two_cycles_1025"] = (1025, i32(np.concatenate([a, b])), i32(np.concatenate([np.roll(a, -1), np.roll(b, -1)])))
    n = (1 << 22) + 17                                                                    # labels and walk past 262 144 tile rows
    out["hyper_4194321"] = (n,) + _random_entries(n, 3000, 22)
    return out
