// concat.hip -- block assembly of tilings (include/pem_spgemm.h): R = [[B00, B01, ..], [B10, ..], ..] from a grid of tilings
// (pem_tiled_concat) and its refresh (pem_tiled_set_values_from_concat).  With row sizes m_a and column sizes n_b, block (a, b) is
// m_a x n_b or null (all empty), R is sum(m_a) x sum(n_b) and stores (ro_a + i, co_b + j) exactly where block (a, b) stores (i, j),
// ro / co the exclusive prefix sums of the sizes; the value is copied bit for bit.
//
// R's order is known in closed form, so no entry is ever sorted.  A block placed at (ro, co) keeps its row-major order, and only
// ro % 16 and co % 16 decide how its tiles are cut: a source tile covers at most 16 consecutive rows and columns of R, so it
// reaches at most 2 x 2 tiles of R.  The grid lives in device tables, not in kernel arguments (a grid of 1 x 1 blocks has hundreds
// of cells): the prefix sums of the row and of the column sizes (int64), a CcCell per cell -- what the walks read of the block, or
// a null marker -- and the scan of the blocks' tile counts, the flat list of all source tiles.  The build is the candidate-tile
// route (tiled_internal.h, extract.hip: sort, pair scan, payload setup, derive_tiled) with these stages:
//   cc_cand_kernel    (emit) one lane per source tile -- its (cell, tile) by a binary search in the scan of the tile counts, the
//                     tile's corner from its key.  First form, before the route: the exact count of R tiles its rows ro + 16p ..
//                     (clipped at the block's last row) and its columns alike reach (1, 2 or 4); after the scan of the counts,
//                     second form: their keys (P << bits_tc) | Q.
//   sort              always (the aligned one-column no-sort path was not built).  Duplicates: a tile of R several source tiles
//                     reach, of one block or of neighbouring blocks.
//   cc_count_kernel   (count) lane r of a candidate: row 16P + r -> (grid row a, local row i) by a binary search in
//                     the row prefix; columns 16Q .. 16Q+15 are cut by the column prefix into at most 16 grid-column segments; for
//                     each segment with a block, the block's row there is at most 16 consecutive columns, so at most two source
//                     tiles, read as one 32-bit mask (row_seg) and shifted into place.  The row's 16-bit mask is kept per candidate
//                     row (rmask, this unit's own buffer); a source tile's bounding box can reach a result tile in which it stores
//                     nothing: such a candidate is no tile of R.
//   cc_fill_kernel    (fill) the same walk from the row's first slot (the kept masks' popcounts give it), the values copied once,
//                     contiguously per row.
// No atomics, and the order of every array is fixed by the grid alone.  ro + i and co + j reach 2^31 - 1: every global index is
// formed in 64 bits and narrowed only once it is a tile index, a 4-bit offset or a block coordinate; launch indices are long long.
//
// Refresh: the pattern is independent of the values.  The first call builds an int2 per entry -- one lane per entry decodes
// (p, q) from the tile key and byte, finds the grid cell by two binary searches and takes src_slot in that block's tile.  Every
// call writes the blocks' current vals pointers into a device table (through kernel arguments, 32 a launch: stream-ordered, no
// host buffer to keep alive) and runs one gather kernel over the entries.
#include "spgemm_internal.h"
#include "tiled_internal.h"
#include <climits>
#include <vector>

using namespace pem;

// ------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------
// what the walks read of a grid cell; s.rowptr == null: a null cell
struct CcCell {
    TileSide s;
    const long long *keys;   // tile_keys
    const void *vals;
};

// the grid on the device: rpre[0 .. grid_rows], cpre[0 .. grid_cols] = exclusive prefix sums of the sizes, cells row-major
struct CcGrid {
    const long long *rpre, *cpre;
    const CcCell *cells;
    int grid_rows, grid_cols;
};

// the strip that holds index x: pre[k] <= x < pre[k + 1] (0 <= x < pre[n]; strips of size 0 hold nothing)
__device__ __forceinline__ int cc_strip(const long long *__restrict__ pre, const int n, const long long x)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (pre[mid + 1] <= x)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// One lane per source tile x of the flat list (tstart = the scan of the cells' tile counts, ncells + 1 values).  The tile's block
// of R is rows ro + 16p .. (clipped at the block's last row) and columns co + 16q .. alike: 1 or 2 tile rows times 1 or 2 tile
// columns.  coff == null: cnt[x] = that count.  Else: the keys at coff[x] .. (coff = the scanned counts).
__global__ void __launch_bounds__(256) cc_cand_kernel(CcGrid G, const long long *__restrict__ tstart, long long ntiles_all, int bits_tc,
                                                      int *__restrict__ cnt, const int *__restrict__ coff, uint64_t *__restrict__ keys)
{
    const long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= ntiles_all) return;
    const int cell = cc_strip(tstart, G.grid_rows * G.grid_cols, x);
    const CcCell &c = G.cells[cell];
    const long long key = c.keys[x - tstart[cell]];
    const long long ro = G.rpre[cell / G.grid_cols], co = G.cpre[cell % G.grid_cols];
    const long long p0 = 16 * (key >> 32), q0 = 16 * (key & 0xFFFFFFFFll);
    const long long p1 = p0 + 15 < c.s.rows ? p0 + 15 : c.s.rows - 1, q1 = q0 + 15 < c.s.cols ? q0 + 15 : c.s.cols - 1;
    const long long P0 = (ro + p0) >> 4, P1 = (ro + p1) >> 4, Q0 = (co + q0) >> 4, Q1 = (co + q1) >> 4;
    if (!coff) {
        cnt[x] = (int)((P1 - P0 + 1) * (Q1 - Q0 + 1));
        return;
    }
    uint64_t *out = keys + coff[x];
    for (long long P = P0; P <= P1; ++P)
        for (long long Q = Q0; Q <= Q1; ++Q) *out++ = ((uint64_t)P << bits_tc) | (uint64_t)Q;
}

// Row p of R in the tile column Q: the walk over the grid columns that reach the tile and, for each with a block, over the block's
// row there.  Returns the row's 16-bit mask.  FILL: also writes the row's entries from slot e on, never at or past e_end.
template <bool FILL, typename VT>
__device__ __forceinline__ unsigned cc_walk(const CcGrid &G, const long long p, const long long Q, const long long r_cols, const int r, int e,
                                            const int e0, const int e_end, const int tile, uint8_t *__restrict__ rowcolidx,
                                            int *__restrict__ headx, VT *__restrict__ vals)
{
    const int a = cc_strip(G.rpre, G.grid_rows, p);
    const int i = (int)(p - G.rpre[a]);   // (below the block's rows <= INT32_MAX)
    const long long q0 = 16 * Q;
    const long long q1 = q0 + 15 < r_cols - 1 ? q0 + 15 : r_cols - 1;
    unsigned rowmask = 0u;
    for (int b = cc_strip(G.cpre, G.grid_cols, q0); b < G.grid_cols && G.cpre[b] <= q1; ++b) {
        const long long lo = G.cpre[b] > q0 ? G.cpre[b] : q0, hi = G.cpre[b + 1] - 1 < q1 ? G.cpre[b + 1] - 1 : q1;
        if (lo > hi) continue;   // (a strip of size 0)
        const CcCell &c = G.cells[(size_t)a * G.grid_cols + b];
        if (!c.s.rowptr) continue;
        const long long llo = lo - G.cpre[b];                           // the block's first column in the tile
        const int tc = (int)(llo >> 4);
        const RowSeg sg = row_seg(c.s, i, tc);
        const unsigned sh = (unsigned)(llo - 16 * (long long)tc);       // ... in the segment: 0 .. 15
        const unsigned width = (unsigned)(hi - lo) + 1u;                // 1 .. 16
        const unsigned bits = (sg.m >> sh) & ((1u << width) - 1u);      // bit k = the block's column llo + k
        const unsigned place = (unsigned)(lo - q0);                     // its column in the tile: 0 .. 15, place + width <= 16
        rowmask |= bits << place;
        if constexpr (FILL) {
            const VT *__restrict__ src = static_cast<const VT *>(c.vals);
            e = write_row_bits(bits, place, r, e, e0, e_end, tile, rowcolidx, headx, vals, [&](const unsigned k) { return src[seg_slot(sg, sh + k)]; });
        }
    }
    return rowmask;
}

// 16 lanes per candidate c, lane = local row r: rmask[16c + r] = the row's mask, cnt[c] = the tile's entries, flag[c] = it has any.
__global__ void __launch_bounds__(256) cc_count_kernel(const uint64_t *__restrict__ keys, long long ncand, CcGrid G, long long r_rows,
                                                       long long r_cols, int bits_tc, uint16_t *__restrict__ rmask, int *__restrict__ cnt,
                                                       int *__restrict__ flag)
{
    const long long c = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int r = threadIdx.x & 15;
    unsigned m = 0u;
    if (c < ncand) {
        const CandKey k = cand_key(keys, c, bits_tc);
        const long long p = 16 * k.P + r;
        if (!k.dup && p < r_rows) m = cc_walk<false, float>(G, p, k.Q, r_cols, r, 0, 0, 0, 0, nullptr, nullptr, nullptr);
        rmask[16 * c + r] = (uint16_t)m;
    }
    cand_count(__popc(m), c, ncand, r, cnt, flag);
}

// 16 lanes per candidate, lane = local row r: the walk again, from the row's first slot
template <typename VT>
__global__ void __launch_bounds__(256) cc_fill_kernel(const uint64_t *__restrict__ keys, long long ncand, CcGrid G, long long r_cols, int bits_tc,
                                                      const uint16_t *__restrict__ rmask, const int *__restrict__ roff, const int *__restrict__ rid,
                                                      long long *__restrict__ tile_keys, int *__restrict__ tile_nnz_ptr,
                                                      uint8_t *__restrict__ rowcolidx, int *__restrict__ headx, VT *__restrict__ vals)
{
    const long long c = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int r = threadIdx.x & 15;
    const int n = c < ncand ? __popc((unsigned)rmask[16 * c + r]) : 0;
    cand_slots(c, ncand, r, n, roff, rid, tile_nnz_ptr, headx, [&](const CandSlots &s) {
        const CandKey k = cand_key(keys, c, bits_tc);
        cand_tile_head(r, s, k.P, k.Q, tile_keys, tile_nnz_ptr);
        if (!n) return;
        cc_walk<true, VT>(G, 16 * k.P + r, k.Q, r_cols, r, s.e, s.e0, s.e1, s.t, rowcolidx, headx, vals);
    });
}

// the refresh map, once.  Entry (p, q) of R is entry (p - ro_a, q - co_b) of block (a, b): the block's tile by mask_find_tile, its
// slot by src_slot.
__global__ void __launch_bounds__(256) cc_map_kernel(const long long *__restrict__ r_keys, long long nt, const int *__restrict__ r_ptr,
                                                     const uint8_t *__restrict__ r_rci, CcGrid G, int2 *__restrict__ map)
{
    for_tile_entries(r_keys, nt, r_ptr, r_rci, [&](const int e, const long long p, const long long q) {   // (p, q below R's rows and columns)
        const int a = cc_strip(G.rpre, G.grid_rows, p), b = cc_strip(G.cpre, G.grid_cols, q);
        const int cell = a * G.grid_cols + b;
        const TileSide &S = G.cells[cell].s;
        int slot = 0;
        if (S.rowptr) {
            const int i = (int)(p - G.rpre[a]), j = (int)(q - G.cpre[b]);
            const int t = mask_find_tile(S.rowptr, S.colidx, i >> 4, j >> 4);
            if (t >= 0) slot = src_slot(S.ptr[t], S.rec[16 * (size_t)t + (i & 15)], (unsigned)(j & 15));
        }
        map[e] = make_int2(cell, slot);
    });
}

// the blocks' vals pointers, 32 cells a launch
struct CcPtrs {
    const void *p[32];
};
__global__ void cc_ptrs_kernel(CcPtrs v, int n, const void **__restrict__ out)
{
    if ((int)threadIdx.x < n) out[threadIdx.x] = v.p[threadIdx.x];
}

// vals[e] = vals_t[map_t[e]] = entry map[e].y of the vals of cell map[e].x: a plain copy through registers
template <typename VT>
__global__ void __launch_bounds__(256) cc_refresh_kernel(const int2 *__restrict__ map, const int *__restrict__ map_t, size_t nnz,
                                                         const void *const *__restrict__ ptrs, VT *__restrict__ vals, VT *__restrict__ vals_t)
{
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    const int2 m = map[e];
    const VT v = static_cast<const VT *>(ptrs[m.x])[m.y];
    vals[e] = v;
    vals_t[map_t[e]] = v;
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
static CcCell cell_of(const pem_tiled *T)
{
    if (!T) return CcCell{TileSide{nullptr, nullptr, nullptr, nullptr, 0, 0}, nullptr, nullptr};
    return CcCell{tile_side(T), T->tile_keys.as<long long>(), T->vals.p};
}

static CcGrid grid_of(const pem_tiled *R)
{
    const Derivation &d = R->derived;
    return CcGrid{d.idx[0].as<long long>(), d.idx[0].as<long long>() + d.op + 1, d.src_tiles.as<CcCell>(), d.op, d.pattern};
}

// the arguments were checked (concat_args_ok): the dimensions and the sum of the blocks' entries fit an int32
template <typename VT>
static pem_status concat_build(pem_ctx *ctx, int grid_rows, int grid_cols, const pem_tiled *const *blocks, const int64_t *row_sizes,
                               const int64_t *col_sizes, int value_bytes, pem_tiled *R, const char *fn)
{
    const size_t ncells = (size_t)grid_rows * grid_cols;
    std::vector<long long> pre((size_t)grid_rows + grid_cols + 2), tstart(ncells + 1);
    std::vector<CcCell> cells(ncells);
    for (size_t k = 0; k < ncells; ++k) cells[k] = cell_of(blocks[k]);
    long long *rpre = pre.data(), *cpre = pre.data() + grid_rows + 1;
    rpre[0] = cpre[0] = 0;
    for (int a = 0; a < grid_rows; ++a) rpre[a + 1] = rpre[a] + row_sizes[a];
    for (int b = 0; b < grid_cols; ++b) cpre[b + 1] = cpre[b] + col_sizes[b];
    long long nnz_all = 0;
    tstart[0] = 0;
    for (size_t k = 0; k < ncells; ++k) {
        tstart[k + 1] = tstart[k] + (blocks[k] ? blocks[k]->ntiles : 0);
        nnz_all += blocks[k] ? blocks[k]->nnz : 0;
    }
    set_tiled_shape(R, value_bytes, (int)rpre[grid_rows], (int)cpre[grid_cols]);
    Derivation &d = R->derived;
    d.kind = Derivation::CONCAT;
    d.op = grid_rows;
    d.pattern = grid_cols;
    d.srcs.resize(ncells);
    for (size_t k = 0; k < ncells; ++k) d.srcs[k] = blocks[k] ? blocks[k]->serial : 0;
    PEM_TRY(zero_flags(ctx));
    PEM_TRY(check_result_entries(ctx, nnz_all, fn));   // (before any kernel: a tile never holds less than one entry)
    const int bits_tc = bits_for((uint64_t)R->tile_cols);
    const size_t ntall = (size_t)tstart[ncells];

    DevBuf d_tstart, coff;   // the scan of the cells' tile counts; per source tile: the R tiles it reaches -> where its keys start
    PEM_TRY(d.idx[0].reserve(sizeof(long long) * pre.size()));
    PEM_TRY(d.src_tiles.reserve(sizeof(CcCell) * ncells));
    PEM_TRY(d_tstart.reserve(sizeof(long long) * (ncells + 1)));
    PEM_TRY(coff.reserve(sizeof(int) * (ntall + 4)));
    PEM_HIP(hipMemcpyAsync(d.idx[0].p, pre.data(), sizeof(long long) * pre.size(), hipMemcpyHostToDevice, ctx->stream));
    PEM_HIP(hipMemcpyAsync(d_tstart.p, tstart.data(), sizeof(long long) * (ncells + 1), hipMemcpyHostToDevice, ctx->stream));
    PEM_HIP(hipMemcpyAsync(d.src_tiles.p, cells.data(), sizeof(CcCell) * ncells, hipMemcpyHostToDevice, ctx->stream));
    PEM_HIP(hipStreamSynchronize(ctx->stream));   // (the host tables go away with this scope, whichever way it is left)
    const CcGrid G = grid_of(R);
    auto cand = [&](int *cnt, const int *off, uint64_t *keys) {   // the counts, then (with their scan) the keys
        PEM_LAUNCH(ctx, cc_cand_kernel, grid_for(ntall, 256), 256, G, d_tstart.as<long long>(), (long long)ntall, bits_tc, cnt, off, keys);
    };
    if (ntall) cand(coff.as<int>(), nullptr, nullptr);
    PEM_TRY(exclusive_scan_i32(ctx, coff.as<int>(), coff.as<int>(), ntall, ctx->d_scalars));
    int64_t tot[1] = {0};
    PEM_TRY(check_candidates(ctx, 1, tot, fn));
    const size_t ncand = (size_t)tot[0];

    DevBuf rmask;   // per candidate: its 16 row masks, from the count to the fill
    PEM_TRY(rmask.reserve(sizeof(uint16_t) * 16 * (ncand + 1)));
    CandidateStages st;
    st.emit = [&](uint64_t *keys) { cand(nullptr, coff.as<int>(), keys); };
    st.count = [&](const uint64_t *keys, int *cnt, int *flag) {
        PEM_LAUNCH(ctx, cc_count_kernel, grid_for(16 * ncand, 256), 256, keys, (long long)ncand, G, (long long)R->rows, (long long)R->cols, bits_tc,
                   rmask.as<uint16_t>(), cnt, flag);
    };
    st.fill = [&](const uint64_t *keys, const int *roff, const int *rid, int *headx) {
        PEM_LAUNCH(ctx, cc_fill_kernel<VT>, grid_for(16 * ncand, 256), 256, keys, (long long)ncand, G, (long long)R->cols, bits_tc, rmask.as<uint16_t>(),
                   roff, rid, R->tile_keys.as<long long>(), R->tile_nnz_ptr.as<int>(), R->rowcolidx.as<uint8_t>(), headx, R->vals.as<VT>());
    };
    // (every entry of every block is exactly one entry of R)
    return tiling_from_candidates(ctx, R, fn, ncand, true, nnz_all, "the blocks'", st);
}

// everything the host knows, in 64 bits, before anything is launched or allocated; *value_bytes = the blocks' value type
static pem_status concat_args_ok(const pem_ctx *ctx, int grid_rows, int grid_cols, const pem_tiled *const *blocks, const int64_t *row_sizes,
                                 const int64_t *col_sizes, int *value_bytes, const char *fn)
{
    if (grid_rows < 1 || grid_cols < 1 || (long long)grid_rows * grid_cols > 0x7FFFFFFFll) {
        set_error("%s: a grid of %d x %d cells (at least 1 x 1, at most INT32_MAX cells)", fn, grid_rows, grid_cols);
        return PEM_E_INVALID;
    }
    long long sum[2] = {0, 0};
    for (int side = 0; side < 2; ++side) {
        const int64_t *sizes = side ? col_sizes : row_sizes;
        for (int k = 0; k < (side ? grid_cols : grid_rows); ++k) {
            if (sizes[k] < 0) {
                set_error("%s: %s size %d is %lld; a size is at least 0", fn, side ? "column" : "row", k, (long long)sizes[k]);
                return PEM_E_INVALID;
            }
            if (sum[side] <= 0x7FFFFFFFll) sum[side] += sizes[k] < 0x80000000ll ? sizes[k] : 0x80000000ll;   // (stops once past the limit: never wraps)
        }
    }
    if (sum[0] > 0x7FFFFFFFll || sum[1] > 0x7FFFFFFFll) {
        set_error("%s: the result would be %lld x %lld (a sum stops once it is past the limit); a dimension holds at most INT32_MAX", fn, sum[0],
                  sum[1]);
        return PEM_E_OVERFLOW;
    }
    const pem_tiled *first = nullptr;
    for (int a = 0; a < grid_rows; ++a)
        for (int b = 0; b < grid_cols; ++b) {
            const pem_tiled *T = blocks[(size_t)a * grid_cols + b];
            if (!T) continue;
            if (T->rows != row_sizes[a] || T->cols != col_sizes[b]) {
                set_error("%s: block (%d, %d) is %d x %d, its cell %lld x %lld", fn, a, b, T->rows, T->cols, (long long)row_sizes[a],
                          (long long)col_sizes[b]);
                return PEM_E_INVALID;
            }
            if (T->tile_rowptr.arena != ctx->arena) {
                set_error("%s: block (%d, %d) was made on another context", fn, a, b);
                return PEM_E_INVALID;
            }
            if (!first) first = T;
            if (T->value_bytes != first->value_bytes) {
                set_error("%s: block (%d, %d) holds %s values, the blocks before it %s", fn, a, b, T->value_bytes == 4 ? "fp32" : "fp64",
                          first->value_bytes == 4 ? "fp32" : "fp64");
                return PEM_E_INVALID;
            }
        }
    if (!first) {
        set_error("%s: every block is null: the result would have no value type", fn);
        return PEM_E_INVALID;
    }
    *value_bytes = first->value_bytes;
    return PEM_OK;
}

extern "C" pem_status pem_tiled_concat(pem_ctx *ctx, int grid_rows, int grid_cols, const pem_tiled *const *blocks, const int64_t *row_sizes,
                                       const int64_t *col_sizes, pem_tiled **out)
{
    const char *fn = "pem_tiled_concat";
    if (out) *out = nullptr;
    if (!ctx || !blocks || !row_sizes || !col_sizes || !out) {
        set_error("%s: null context, blocks, sizes or output", fn);
        return PEM_E_INVALID;
    }
    int value_bytes = 8;
    PEM_TRY(concat_args_ok(ctx, grid_rows, grid_cols, blocks, row_sizes, col_sizes, &value_bytes, fn));
    return build_derived(ctx, out, [&](pem_tiled *R) {
        pem_status s = value_bytes == 4 ? concat_build<float>(ctx, grid_rows, grid_cols, blocks, row_sizes, col_sizes, value_bytes, R, fn)
                                        : concat_build<double>(ctx, grid_rows, grid_cols, blocks, row_sizes, col_sizes, value_bytes, R, fn);
        (void)hipStreamSynchronize(ctx->stream);   // (the temporaries went back to the arena)
        return s;
    });
}

// once: the pointer table and every entry's (cell, slot).  The build's cell table still holds: the serials were checked, and a
// tiling's structure arrays never move (its vals pointer, which they say may, is not read here).
static pem_status concat_map(pem_ctx *ctx, pem_tiled *t)
{
    const size_t nnz = (size_t)t->nnz, nt = (size_t)t->ntiles;
    PEM_TRY(t->derived.map.reserve(sizeof(int2) * (nnz + 1)));
    PEM_TRY(t->derived.idx[1].reserve(sizeof(void *) * t->derived.srcs.size()));
    PEM_LAUNCH(ctx, cc_map_kernel, grid_for((nt + 63) / 64 * 64, 256), 256, t->tile_keys.as<long long>(), (long long)nt, t->tile_nnz_ptr.as<int>(),
               t->rowcolidx.as<uint8_t>(), grid_of(t), t->derived.map.as<int2>());
    return PEM_OK;
}

template <typename VT>
static void concat_refresh(pem_ctx *ctx, pem_tiled *t, const pem_tiled *const *blocks)
{
    const size_t ncells = t->derived.srcs.size(), nnz = (size_t)t->nnz;
    const void **ptrs = t->derived.idx[1].as<const void *>();
    for (size_t k0 = 0; k0 < ncells; k0 += 32) {
        CcPtrs v;
        const int n = ncells - k0 < 32 ? (int)(ncells - k0) : 32;
        for (int k = 0; k < 32; ++k) v.p[k] = k < n && blocks[k0 + k] ? blocks[k0 + k]->vals.p : nullptr;
        PEM_LAUNCH(ctx, cc_ptrs_kernel, 1, 32, v, n, ptrs + k0);
    }
    PEM_LAUNCH(ctx, cc_refresh_kernel<VT>, grid_for(nnz, 256), 256, t->derived.map.as<int2>(), t->vmap_t.as<int>(), nnz,
               (const void *const *)ptrs, t->vals.as<VT>(), t->vals_t.as<VT>());
}

extern "C" pem_status pem_tiled_set_values_from_concat(pem_ctx *ctx, pem_tiled *t, int nblocks, const pem_tiled *const *blocks)
{
    const char *fn = "pem_tiled_set_values_from_concat";
    if (!ctx || !t || !blocks) {
        set_error("%s: null context, tiling or blocks", fn);
        return PEM_E_INVALID;
    }
    const Derivation &d = t->derived;
    bool same = d.kind == Derivation::CONCAT && nblocks >= 0 && (size_t)nblocks == d.srcs.size();
    for (int k = 0; same && k < nblocks; ++k) same = (blocks[k] ? blocks[k]->serial : 0) == d.srcs[k];
    if (!same) {
        set_error("%s: the tiling was not made by pem_tiled_concat from this grid of blocks (in this order, nulls where it had nulls)", fn);
        return PEM_E_INVALID;
    }
    const bool f32 = t->value_bytes == 4;
    return refresh_derived(
        ctx, t, [&] { return concat_map(ctx, t); },
        [&] { f32 ? concat_refresh<float>(ctx, t, blocks) : concat_refresh<double>(ctx, t, blocks); });
}
