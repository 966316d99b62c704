"""Tile-aligned compaction: host references whose cost depends on the entries, never on the dimensions.

An empty tile row or tile column of an operand adds nothing to any operation of this project: no tile, no product, no pair, no
entry.  So a matrix with its empty 16-line blocks squeezed out computes the same per-entry, per-tile and per-pair arrays, and only
the arrays that are INDEXED by a tile line or that HOLD a line index change -- the first by insertion of empty lines, the second
by a monotone renaming.  The map keeps the position inside a tile (idx & 15), so masks, in-tile row pointers and in-tile indices
are untouched, and it is monotone, so every sort order (tiles by row then column, entries inside a tile, the ascending-k fma chain
of a product) is the order of the uncompacted run: values stay comparable bit for bit.  For a square product A*A rows and columns
go through ONE map over the union of the used tile rows and tile columns, so that the inner index k is renamed once.

tests/test_compact_cpu.py proves the lifted results equal to the plain oracle's where that still runs.
"""
import numpy as np

T_NAMES = ["tile_keys", "tile_nnz_ptr", "masks", "rowptr", "rowcolidx", "vals", "masks_t", "tile_rowptr", "tile_colidx",
           "tile_colptr", "tile_rowidx", "tile_offsets"]


class LineMap:
    """the monotone map of one dimension: used[k] is the original tile line of compacted tile line k"""

    def __init__(self, used, dim):
        self.used = np.asarray(used, dtype=np.int64)
        assert self.used.ndim == 1 and (len(self.used) == 0 or (np.all(np.diff(self.used) > 0) and self.used[0] >= 0))
        self.dim = int(dim)
        self.tiles = (self.dim + 15) // 16
        assert len(self.used) == 0 or self.used[-1] < self.tiles
        self.cdim = max(16 * len(self.used), 1)      # (a dimension of 0 is no matrix: an all-empty one keeps one line)

    def fwd(self, idx):
        """original index -> compacted index (every idx must lie in a used tile line)"""
        idx = np.asarray(idx, dtype=np.int64)
        rank = np.searchsorted(self.used, idx >> 4)
        assert np.array_equal(self.used[rank], idx >> 4), "an index outside the used tile lines"
        return (rank * 16 + (idx & 15)).astype(np.int32)

    def inv(self, idx):
        """compacted index -> original index"""
        idx = np.asarray(idx, dtype=np.int64)
        return (self.used[idx >> 4] * 16 + (idx & 15)).astype(np.int32)

    def inv_tile(self, t):
        """compacted tile line -> original tile line"""
        return self.used[np.asarray(t, dtype=np.int64)].astype(np.int32)

    def expand_ptr(self, ptr_c):
        """a pointer array over the compacted tile lines -> the one over all original tile lines (O(tiles): small cases only)"""
        cnt = np.zeros(self.tiles, np.int64)
        cnt[self.used] = np.diff(ptr_c[:len(self.used) + 1])
        return np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)

    def expand_line_ptr(self, ptr_c):
        """a pointer array over the compacted LINES (16 per tile line, a CSR rowptr) -> the one over the original `dim` lines"""
        cnt = np.zeros(self.tiles * 16, np.int64)
        d = np.diff(ptr_c)
        k = np.arange(min(len(d), 16 * len(self.used)), dtype=np.int64)
        cnt[self.used[k >> 4] * 16 + (k & 15)] = d[:len(k)]
        assert not cnt[self.dim:].any()
        return np.concatenate([[0], np.cumsum(cnt[:self.dim])]).astype(np.int32)

    def ptr_matches(self, got, ptr_c):
        """`got` (a pointer array over all original tile lines) == expand_ptr(ptr_c), decided from its values at the used lines:
        a nondecreasing array that starts at 0, ends at the total and equals ptr_c[k], ptr_c[k + 1] at used[k], used[k] + 1 is pinned
        between them everywhere else.  Builds no reference of the original length."""
        ptr_c = np.asarray(ptr_c)[:len(self.used) + 1]
        if got.dtype != ptr_c.dtype or got.shape != (self.tiles + 1,) or got[0] != 0 or got[-1] != ptr_c[-1]:
            return False
        if not (np.array_equal(got[self.used], ptr_c[:-1]) and np.array_equal(got[self.used + 1], ptr_c[1:])):
            return False
        return bool(np.all(got[1:] >= got[:-1]))


def compact(tile_idx, dim):
    """tile_idx: the tile lines in use (idx >> 4 of every entry, any order, repeats allowed) -> the LineMap of that dimension"""
    return LineMap(np.unique(np.asarray(tile_idx, dtype=np.int64)), dim)


def identity(dim):
    return LineMap(np.arange((int(dim) + 15) // 16, dtype=np.int64), dim)


def compact_rows(rows, cols, I, J):
    """A*A^T: compact A's rows; its columns (the inner index) stay -> (rmap, cmap)"""
    return compact(np.asarray(I, np.int64) >> 4, rows), identity(cols)


def compact_square(n, I, J):
    """A*A: ONE map over the union of the used tile rows and tile columns -> (map, map)"""
    m = compact(np.concatenate([np.asarray(I, np.int64) >> 4, np.asarray(J, np.int64) >> 4]), n)
    return m, m


class LiftedTiled:
    """an oracle.Tiled of the compacted matrix, seen in the original index space.  rmap / cmap: the maps of the TILED matrix's rows
    and columns (for a tiling made with transpose=True: the source's column map and row map).  The two pointer arrays over tile lines
    stay compacted: compare with matches(), or expand them (small cases) with array()."""

    def __init__(self, o, rmap, cmap):
        self.o, self.rmap, self.cmap = o, rmap, cmap
        self.rows, self.cols, self.nnz, self.ntiles = rmap.dim, cmap.dim, o.nnz, o.ntiles
        self.tile_rows, self.tile_cols = rmap.tiles, cmap.tiles

    def array(self, name):
        o = self.o
        if name == "tile_keys":
            k = o.tile_keys
            return (self.rmap.inv_tile(k >> 32).astype(np.int64) << 32) | self.cmap.inv_tile(k & 0xFFFFFFFF).astype(np.int64)
        if name == "tile_colidx":
            return self.cmap.inv_tile(o.tile_colidx)
        if name == "tile_rowidx":
            return self.rmap.inv_tile(o.tile_rowidx)
        if name == "tile_rowptr":
            return self.rmap.expand_ptr(o.tile_rowptr)
        if name == "tile_colptr":
            return self.cmap.expand_ptr(o.tile_colptr)
        return getattr(o, name)

    def matches(self, name, got):
        if name == "tile_rowptr":
            return self.rmap.ptr_matches(got, self.o.tile_rowptr)
        if name == "tile_colptr":
            return self.cmap.ptr_matches(got, self.o.tile_colptr)
        want = self.array(name)
        return got.dtype == want.dtype and np.array_equal(got, want)


def lift_plan_arrays(arrays, rmap, cmap, expand=True):
    """plan arrays of the compacted product (an oracle.Plan's, or prune_ref.expected's dict) -> the original index space.  rmap: A's
    row map, cmap: B's column map.  expand=False leaves c_tile_rowptr compacted (compare it with rmap.ptr_matches)."""
    out = dict(arrays)
    out["c_tile_rowidx"] = rmap.inv_tile(arrays["c_tile_rowidx"])
    out["c_tile_colidx"] = cmap.inv_tile(arrays["c_tile_colidx"])
    if expand:
        out["c_tile_rowptr"] = rmap.expand_ptr(arrays["c_tile_rowptr"])
    return out


def lift_coo(r, c, v, rmap, cmap):
    return rmap.inv(r), cmap.inv(c), v


def lift_csr(rp, ci, v, rmap, cmap):
    """(O(rows): small cases only)"""
    return rmap.expand_line_ptr(rp), cmap.inv(ci), v


def csr_to_coo(rp, ci, v):
    return np.repeat(np.arange(len(rp) - 1, dtype=np.int32), np.diff(rp)), ci, v


class Product:
    """A*A^T (case[5] true: A's rows compacted) or the square A*A (one map for rows and columns) of a matgen case, computed by the
    oracle on the compacted operands.  A, B: LiftedTiled; op: the oracle.Plan of the compacted product (None with plan=False);
    rmap / cmap: the maps of C's rows and columns."""

    def __init__(self, oracle, case, plan=True):
        rows, cols, I, J, V, tr = case
        if tr:
            rmap, kmap = compact_rows(rows, cols, I, J)
        else:
            assert rows == cols, "a non-square A*B needs a map per dimension: not needed so far"
            rmap, kmap = compact_square(rows, I, J)
        self.cI, self.cJ, self.V, self.tr = rmap.fwd(I), kmap.fwd(J), np.asarray(V, np.float64), tr
        self.crows, self.ccols = rmap.cdim, kmap.cdim
        self.oA = oracle.Tiled(self.crows, self.ccols, self.cI, self.cJ, self.V, False)
        self.oB = oracle.Tiled(self.crows, self.ccols, self.cI, self.cJ, self.V, True) if tr else self.oA
        self.A = LiftedTiled(self.oA, rmap, kmap)
        self.B = LiftedTiled(self.oB, kmap, rmap) if tr else self.A
        self.rmap, self.cmap = rmap, (rmap if tr else kmap)
        self.oracle = oracle
        self.op = oracle.Plan(self.oA, self.oB) if plan else None

    def csr_spgemm_coo(self, f32=False, values=None):
        """the serial CSR Gustavson product of the compacted operands as lifted sorted COO (values: another V, in the case's order)"""
        V = self.V if values is None else np.asarray(values, np.float64)
        sa = self.oracle.Csr(self.crows, self.ccols, self.cI, self.cJ, V, False)
        sb = self.oracle.Csr(self.crows, self.ccols, self.cI, self.cJ, V, self.tr) if self.tr else sa
        rp, ci, v = self.oracle.csr_spgemm(sa, sb, 1, f32=f32).arrays()
        return lift_coo(*csr_to_coo(rp, ci, v), self.rmap, self.cmap), (rp, ci, v)


def row_products(arrays):
    """products per (compacted) tile row of a plan: what step 1's row classification bins by"""
    return np.diff(arrays["pairs_offset"][arrays["c_tile_rowptr"]].astype(np.int64))


def product_coo(oracle, n, a, b, f32=False):
    """the serial CSR Gustavson product of two square n x n COO operands (I, J, V) as sorted COO in the original index space: ONE map
    over the used tile lines of both operands, so the inner index is renamed once and the fma chain keeps its order"""
    m = compact(np.concatenate([np.asarray(x, np.int64) >> 4 for x in (a[0], a[1], b[0], b[1])]), n)
    sa = oracle.Csr(m.cdim, m.cdim, m.fwd(a[0]), m.fwd(a[1]), np.asarray(a[2], np.float64), False)
    sb = oracle.Csr(m.cdim, m.cdim, m.fwd(b[0]), m.fwd(b[1]), np.asarray(b[2], np.float64), False)
    return lift_coo(*csr_to_coo(*oracle.csr_spgemm(sa, sb, 1, f32=f32).arrays()), m, m)


def lifted_tiled(oracle, rows, cols, I, J, V, transpose=False):
    """the LiftedTiled of one matrix (rows and columns compacted on their own; transpose: the tiling of the transposed matrix)"""
    rmap, cmap = compact(np.asarray(I, np.int64) >> 4, rows), compact(np.asarray(J, np.int64) >> 4, cols)
    o = oracle.Tiled(rmap.cdim, cmap.cdim, rmap.fwd(I), cmap.fwd(J), V, transpose)
    return LiftedTiled(o, cmap, rmap) if transpose else LiftedTiled(o, rmap, cmap)


class IndexMap:
    """plain (not tile-aligned) compaction of one index space, for the vector operations, whose references know no tiles: a line
    without an entry gives its output the start value -- or leaves it as it is -- and its input is never read, so the reference runs
    on the used lines only and scatter() puts its outputs back.  used: the sorted indices that hold an entry (rows and columns of a
    square matrix together, so that one map serves both orientations)."""

    def __init__(self, idx, dim):
        self.used = np.unique(np.asarray(idx, np.int64))
        self.dim, self.cdim = int(dim), len(self.used)

    def fwd(self, idx):
        rank = np.searchsorted(self.used, np.asarray(idx, np.int64))
        assert np.array_equal(self.used[rank], idx)
        return rank

    def gather(self, full):
        return np.ascontiguousarray(np.asarray(full)[self.used])

    def scatter(self, compacted, fill):
        """fill: a scalar (the start value) or the full-length old vector"""
        compacted = np.asarray(compacted)
        out = np.full(self.dim, fill, compacted.dtype) if np.ndim(fill) == 0 else np.array(fill, compacted.dtype)
        out[self.used] = compacted
        return out

    def csr(self, I, J, V):
        """the sorted CSR (int64 rowptr, int64 colidx, vals) of the compacted square matrix"""
        i, j = self.fwd(I), self.fwd(J)
        o = np.lexsort((j, i))
        rp = np.zeros(self.cdim + 1, np.int64)
        np.cumsum(np.bincount(i, minlength=self.cdim), out=rp[1:])
        return rp, j[o], np.asarray(V)[o]


# ---- the graph routines and the solves: references on the lines that carry an off-diagonal entry ------------------------------------
# A vertex without an off-diagonal entry has no neighbour, a row without one no fma: what the operation gives it is known without
# running anything, and the others never look at it.  The map is monotone, so "ties to the lower index", the ascending roots and
# the ascending-j fma chains keep their order.  tests/test_compact_cpu.py holds every rule below equal to the plain reference.

def offdiag_map(n, I, J):
    """the IndexMap over the indices that carry an off-diagonal entry, as a row or as a column"""
    I, J = np.asarray(I, np.int64), np.asarray(J, np.int64)
    off = I != J
    return IndexMap(np.concatenate([I[off], J[off]]), n)


def compact_pattern(m, I, J):
    """the off-diagonal entries in the compacted index space: (I, J) int32, in the input's order"""
    I, J = np.asarray(I, np.int64), np.asarray(J, np.int64)
    off = I != J
    return m.fwd(I[off]).astype(np.int32), m.fwd(J[off]).astype(np.int32)


def compact_system(m, I, J, V):
    """(csr, kept): the sorted CSR of the rows in m.used (their columns lie in m.used too: an off-diagonal entry puts both of its
    indices there) and the bool mask of those entries in the (row, col) order of the whole matrix"""
    I, J = np.asarray(I, np.int64), np.asarray(J, np.int64)
    o = np.lexsort((J, I))
    kept = np.isin(I[o], m.used)
    return m.csr(I[o][kept], J[o][kept], np.asarray(V)[o][kept]), kept


def lift_colours(m, colours_c):
    """a vertex without a neighbour takes colour 0 in round 1; ncolours and rounds are the compacted run's (which has a vertex)"""
    return m.scatter(colours_c, 0)


def lift_mis(m, in_set_c, count_c):
    """a vertex without a neighbour is in every maximal independent set, at either distance -> (in_set, count)"""
    return m.scatter(in_set_c, 1), int(count_c) + m.dim - m.cdim


def lift_aggregate(m, agg_c, roots_c, nc_c):
    """(agg, roots, naggregates): a vertex without a neighbour is the root of its own aggregate; the roots are numbered in ascending
    vertex order, so agg[v] is the rank of v's root among all of them"""
    root_of = np.arange(m.dim, dtype=np.int64)
    if m.cdim:
        root_of[m.used] = m.used[np.asarray(roots_c, np.int64)[np.asarray(agg_c, np.int64)]]
    is_root = np.ones(m.dim, bool)
    is_root[m.used] = False
    is_root[m.used[np.asarray(roots_c, np.int64)]] = True
    roots = np.flatnonzero(is_root)
    rank = np.cumsum(is_root) - 1
    assert len(roots) == int(nc_c) + m.dim - m.cdim
    return rank[root_of].astype(np.int32), roots.astype(np.int32), len(roots)


def lift_solution(m, x_c, b, diag=None):
    """a triangular solve's x: a row without an off-diagonal entry is b_i / a_ii, one division in the value type (diag: the full
    diagonal; None under unit_diag: b_i), the others the compacted system's"""
    b = np.asarray(b)
    with np.errstate(all="ignore"):
        rest = b.copy() if diag is None else b / np.asarray(diag, b.dtype)
    return m.scatter(np.asarray(x_c, b.dtype), rest)


def lift_factor(kept, f_c, V_sorted):
    """ILU(0)'s values in the (row, col) order of the whole matrix: a row without an off-diagonal entry keeps its a_ii (no fma, no
    division), the others take the compacted factor's, whose CSR order is theirs"""
    out = np.array(V_sorted)
    out[kept] = f_c
    return out


def lift_index(m, idx_c, none=-1):
    """an index output over the compacted lines (an argmin's column, a BFS parent): the indices renamed back, `none` kept, absent lines
    `none` (or, `none` a full-length vector, what they held)"""
    idx_c = np.asarray(idx_c, np.int64)
    back = np.where(idx_c >= 0, m.used[np.maximum(idx_c, 0)], idx_c).astype(np.int32) if m.cdim else idx_c.astype(np.int32)
    return m.scatter(back, none)
