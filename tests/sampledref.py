"""Independent numpy statement of the sampled sparse product of a tiling (include/pem_spgemm.h pem_tiled_sampled_mxm /
pem_tiled_set_values_sampled_mxm): for every stored position e = (i_e, j_e) of the pattern

    R_e = the left fold, in ascending k, over the k where A(i_e, k) and B(k, j_e) are both stored, of A(i_e, k) (x) B(k, j_e)

from the semiring's start value -- or from the entry's old value with accumulate (lor_land: from old != 0).  The folds are
sddmmref's (plus_pair: acc + 1 per k).  The matched (a_k, b_k) pairs of every entry are listed once from the CSR forms (`match`),
in ascending k, as a ragged array; plus_times then goes through mxvref._plus_times with that ragged row pointer, the way sddmmref
does with its fixed k: entry e is row e of a matrix holding its a_k, the x vector holds its b_k, and the oracle's product returns
every fma chain -- with the [y | A] * [1 ; x] start for accumulate.  The other semirings fold with mxvref._fold.

Matrices are CSR triples (rowptr, colidx, vals) with ascending columns.  B is the n x p matrix of the product whatever the
call's transpose_b: a test that passes B^T to the device passes B here.

The file also holds the generators the sampled tests add to matgen.cases() (`generators`).
"""
import numpy as np

import mxvref as mr
from matgen import cases

SEMIRINGS = mr.SEMIRINGS
START = mr.MXV_START


def csr(rows, cols, I, J, V):
    """sorted CSR of a COO matrix without duplicates"""
    I, J = np.asarray(I, np.int64), np.asarray(J, np.int64)
    o = np.lexsort((J, I))
    rp = np.zeros(rows + 1, np.int64)
    np.cumsum(np.bincount(I, minlength=rows), out=rp[1:])
    return rp, J[o], np.asarray(V)[o]


def rows_of(rp):
    rp = np.asarray(rp, np.int64)
    return np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))


def match(I, J, A, B, n, p):
    """(rp, ia, ib): entry e's matched pairs are ia[rp[e] : rp[e + 1]] (slots in A's vals) and ib[..] (slots in B's vals), in
    ascending k.  A is m x n, B is n x p."""
    I, J = np.asarray(I, np.int64), np.asarray(J, np.int64)
    arp, aci, _ = A
    arp, aci = np.asarray(arp, np.int64), np.asarray(aci, np.int64)
    brp, bci, _ = B
    # B by column: the keys j * n + k of its entries, sorted, and each key's slot in B's vals
    bk = np.asarray(bci, np.int64) * n + rows_of(brp)
    bo = np.argsort(bk, kind="stable")
    bk = bk[bo]
    nnz = len(I)
    alen = (arp[1:] - arp[:-1])[I] if nnz else np.zeros(0, np.int64)
    total = int(alen.sum())
    e = np.repeat(np.arange(nnz, dtype=np.int64), alen)
    first = np.repeat(np.cumsum(alen) - alen, alen)
    ai = arp[I][e] + (np.arange(total, dtype=np.int64) - first)   # row i_e of A, ascending k
    key = J[e] * n + aci[ai]
    pos = np.searchsorted(bk, key)
    hit = pos < len(bk)
    hit[hit] = bk[pos[hit]] == key[hit]
    rp = np.zeros(nnz + 1, np.int64)
    np.cumsum(np.bincount(e[hit], minlength=nnz), out=rp[1:])
    return rp, ai[hit], bo[pos[hit]]


def fold(matched, A, B, semiring, dtype, old=None, oracle=None):
    """the values of every entry from its matched pairs; old: the entries' old values (accumulate) or None"""
    dtype = np.dtype(dtype).type
    rp, ia, ib = matched
    nnz, total = len(rp) - 1, len(ia)
    a, b = np.asarray(A[2]).astype(dtype)[ia], np.asarray(B[2]).astype(dtype)[ib]
    if old is not None:
        old = np.asarray(old, dtype)
    if semiring == "plus_times":
        if nnz == 0:
            return np.zeros(0, dtype)
        if total == 0:
            return np.zeros(nnz, dtype) if old is None else old.copy()
        if oracle is None:
            raise ValueError("plus_times needs the oracle (the fma chain)")
        return mr._plus_times(oracle, nnz, total, rp, np.arange(total, dtype=np.int64), a, b, dtype, old)
    if old is None:
        acc = np.full(nnz, START[semiring], dtype)
    else:
        acc = (old != 0).astype(dtype) if semiring == "lor_land" else old.copy()
    one = dtype(1)
    with np.errstate(all="ignore"):
        if semiring == "plus_pair":
            return mr._fold(rp, np.zeros(total, dtype), lambda x, t: x + one, acc).astype(dtype)
        if semiring == "lor_land":
            return mr._fold(rp, ((a != 0) & (b != 0)), lambda x, t: np.where(t, one, x), acc).astype(dtype)
        if semiring == "min_plus":
            return mr._fold(rp, a + b, np.fmin, acc).astype(dtype)
        if semiring == "max_plus":
            return mr._fold(rp, a + b, np.fmax, acc).astype(dtype)
        if semiring == "max_times":
            return mr._fold(rp, a * b, np.fmax, acc).astype(dtype)
    raise ValueError(semiring)


def sampled(I, J, A, B, n, p, semiring, dtype, old=None, oracle=None):
    """R_e for every entry (I[e], J[e]) of the pattern, in that order"""
    return fold(match(I, J, A, B, n, p), A, B, semiring, dtype, old, oracle)


def transpose(rows, cols, M):
    """CSR of the cols x rows transpose"""
    rp, ci, v = M
    return csr(cols, rows, ci, rows_of(rp), v)


def split_columns(A, B, n1, p):
    """(A1, B1), (A2, B2): A's columns and B's rows below n1 and from n1 on; the shapes stay (the other part is just not stored)"""
    arp, aci, av = A
    brp, bci, bv = B
    m, n = len(arp) - 1, len(brp) - 1
    ai, bi = rows_of(arp), rows_of(brp)
    lo_a, lo_b = np.asarray(aci) < n1, bi < n1
    return ((csr(m, n, ai[lo_a], aci[lo_a], av[lo_a]), csr(n, p, bi[lo_b], bci[lo_b], bv[lo_b])),
            (csr(m, n, ai[~lo_a], aci[~lo_a], av[~lo_a]), csr(n, p, bi[~lo_b], bci[~lo_b], bv[~lo_b])))


# ------------------------------------------------------------------------------------------------------------------------------
# the generators of the sampled tests: name -> dict(m, n, p, S=(I, J), A=(I, J, V), B=(I, J, V)); A is m x n, B is n x p, S is m x p
# ------------------------------------------------------------------------------------------------------------------------------
def _vals(rng, n):
    return rng.integers(1, 10, n) * rng.choice([-0.25, 0.25, 0.5, 1.5], n)


def _rand(rng, rows, cols, nnz):
    k = rng.choice(rows * cols, size=min(nnz, rows * cols), replace=False)
    return (k // cols).astype(np.int32), (k % cols).astype(np.int32)


def _tiles(rng, tile_rows, tile_cols, density):
    """entries of the listed 16 x 16 tiles at about `density`, every tile non-empty"""
    I, J = [], []
    for tr, tc in zip(tile_rows, tile_cols):
        m = rng.random((16, 16)) < density
        m[rng.integers(0, 16), rng.integers(0, 16)] = True
        r, c = np.nonzero(m)
        I.append(16 * tr + r)
        J.append(16 * tc + c)
    return np.concatenate(I).astype(np.int32), np.concatenate(J).astype(np.int32)


# long_lists: where the common keys sit in the longer (130 tiles) and in the shorter (70 tiles) list
LONG_POS, SHORT_POS = (0, 63, 64, 65, 129), (0, 63, 64, 65, 69)


def long_list_keys():
    """the two ascending tile-index lists of long_lists: 130 and 70 keys with the common ones at LONG_POS / SHORT_POS"""
    a = 10 * np.arange(130)                                                   # multiples of 10
    b = np.concatenate([[0], 10 * np.arange(62) + 5, a[[63, 64, 65]], [655, 665, 675], [a[129]]])   # B's own keys end in 5
    assert len(b) == 70 and np.all(np.diff(b) > 0)
    common, ia, ib = np.intersect1d(a, b, return_indices=True)
    assert tuple(ia) == LONG_POS and tuple(ib) == SHORT_POS
    return a, b


def generators():
    rng = np.random.default_rng(20261019)
    out = {}

    def put(name, m, n, p, S, A, B):
        out[name] = dict(m=m, n=n, p=p, S=S, A=A + (_vals(rng, len(A[0])),), B=B + (_vals(rng, len(B[0])),))

    # one 16-row A with 130 non-empty tiles against a B whose tile column has 70: the walk (70 keys) and the search (130) both
    # cross the 64-key chunk, with matches at the chunk's edges; and the same with the roles swapped (A's list is the shorter)
    a, b = long_list_keys()
    n = 16 * (int(a[-1]) + 1)
    AI, AJ = _tiles(rng, np.zeros(130, int), a, 0.3)
    BI, BJ = _tiles(rng, b, np.zeros(70, int), 0.3)
    put("long_lists", 16, n, 16, _rand(rng, 16, 16, 100), (AI, AJ), (BI, BJ))
    put("long_lists_swapped", 16, n, 16, _rand(rng, 16, 16, 100), (BJ, BI), (AJ, AI))
    # a pattern tile with 256 entries (four accumulators in a lane of a 64-lane group) against 3-tile lists
    put("full_tile", 16, 48, 16, tuple(x.ravel().astype(np.int32) for x in np.meshgrid(np.arange(16), np.arange(16), indexing="ij")),
        _tiles(rng, [0, 0, 0], [0, 1, 2], 0.4), _tiles(rng, [0, 1, 2], [0, 0, 0], 0.4))
    # pattern tiles of 1, 63, 64 and 65 entries in one tile row
    SI, SJ = [], []
    for tc, cnt in enumerate((1, 63, 64, 65)):
        i, j = _rand(rng, 16, 16, cnt)
        SI.append(i)
        SJ.append(16 * tc + j)
    put("thin_tiles", 16, 32, 64, (np.concatenate(SI), np.concatenate(SJ)), _rand(rng, 16, 32, 200), _rand(rng, 32, 64, 700))
    # the tiles match, but A stores only even k and B only odd k: every entry holds the start value
    ai, aj = _rand(rng, 32, 32, 400)
    bi, bj = _rand(rng, 32, 32, 400)
    put("no_common_k", 32, 32, 32, _rand(rng, 32, 32, 300), (ai[aj % 2 == 0], aj[aj % 2 == 0]), (bi[bi % 2 == 1], bj[bi % 2 == 1]))
    # pattern tiles whose A tile row is empty (tile row 1) and whose B tile column is empty (tile column 2)
    ai, aj = _rand(rng, 48, 48, 500)
    bi, bj = _rand(rng, 48, 48, 500)
    put("empty_sides", 48, 48, 48, _rand(rng, 48, 48, 600), (ai[ai // 16 != 1], aj[ai // 16 != 1]), (bi[bj // 16 != 2], bj[bj // 16 != 2]))
    put("ragged", 37, 53, 29, _rand(rng, 37, 29, 400), _rand(rng, 37, 53, 500), _rand(rng, 53, 29, 450))
    return out


def triangle_graph(nv=40, nedges=200, seed=5):
    """(n, I, J): the symmetric adjacency pattern of a random graph without loops"""
    rng = np.random.default_rng(seed)
    i, j = rng.integers(0, nv, nedges), rng.integers(0, nv, nedges)
    keep = i != j
    k = np.unique(np.concatenate([i[keep] * nv + j[keep], j[keep] * nv + i[keep]]))
    return nv, (k // nv).astype(np.int32), (k % nv).astype(np.int32)


def symmetrised(n, I, J):
    """the pattern of M + M^T without the diagonal"""
    I, J = np.asarray(I, np.int64), np.asarray(J, np.int64)
    keep = I != J
    k = np.unique(np.concatenate([I[keep] * n + J[keep], J[keep] * n + I[keep]]))
    return (k // n).astype(np.int32), (k % n).astype(np.int32)


def triangles(n, I, J):
    """the triangle count of a symmetric pattern without loops: trace(A^3) / 6 in integer numpy"""
    M = np.zeros((n, n), np.int64)
    M[np.asarray(I, np.int64), np.asarray(J, np.int64)] = 1
    assert np.array_equal(M, M.T) and not M.diagonal().any()
    t = int(np.trace(M @ M @ M))
    assert t % 6 == 0
    return t // 6


CASES = cases()
BIG = ("wide_tilecols", "k64_bins", "hub_tile_2100_AAt", "blockrows_10000")
SMALL = sorted(n for n in CASES if n not in BIG)
GENS = generators()


def problem(name):
    """(m, n, p, (SI, SJ), A, B) of a matgen case or a generator: S's pattern in CSR order and the CSR triples of A (m x n) and B
    (n x p).  A matgen case gives A, B = A or A^T as its AAt flag says, and S = A's pattern wherever A's shape is the product's; a
    non-square AAt case has an m x m product, so its S is a random m x m pattern with A's entry count."""
    if name in GENS:
        g = GENS[name]
        m, n, p = g["m"], g["n"], g["p"]
        A, B = csr(m, n, *g["A"]), csr(n, p, *g["B"])
        SI, SJ = g["S"]
    else:
        m, n, I, J, V, aat = CASES[name]
        A = csr(m, n, I, J, V)
        B = transpose(m, n, A) if aat else A
        p = m if aat else n
        if p == n:
            SI, SJ = I, J
        else:
            k = np.random.default_rng(len(I)).choice(m * p, size=min(len(I), m * p), replace=False)
            SI, SJ = k // p, k % p
    srp, sci, _ = csr(m, p, SI, SJ, np.zeros(len(SI)))
    return m, n, p, (rows_of(srp), sci), A, B
