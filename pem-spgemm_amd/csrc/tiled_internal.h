// tiled_internal.h -- what the units that build, refresh or look up a tiling share (convert.hip, values.hip, chain.hip, mask.hip,
// ewise.hip, select.hip, topk.hip, extract.hip, assign.hip, apply.hip, kron.hip, build.hip, concat.hip, sddmm.hip, sampled.hip, trsv.hip, ilu0.hip).  A derived tiling (chain.hip, ewise.hip, select.hip, extract.hip, assign.hip, apply.hip, kron.hip, build.hip, concat.hip, ilu0.hip) is built by build_derived around its route: the shape
// (set_tiled_shape), the payload arrays (reserve_payload, begin_payload), the route's payload kernels, derive_tiled; its
// provenance is pem_tiled::derived (pem_internal.h), and refresh_derived runs its pem_tiled_set_values_from_*.  build.hip shares the
// HEAD of pem_tiled_from_coo* (coo_sort_keys, then the radix sort) and this tail; its payload kernel is its own, because it compacts the
// sorted positions to entries where convert.hip's conv_fill_kernel writes one value per position.
// extract.hip, kron.hip and concat.hip build their result from a list of candidate result tiles: that route is written once, on the
// host (check_candidates, tiling_from_candidates) and on the device (cand_key, cand_count, cand_slots, cand_tile_head, write_row_bits); chain.hip's
// scatter uses the device half.  The refresh-map kernels of these units and of assign.hip are for_tile_entries around their own body.
#pragma once
#include "pem_internal.h"
#include <chrono>
#include <climits>
#include <functional>
#include <memory>
#include <type_traits>

namespace pem {

// value_bytes, rows, cols and the tile grid (tile_rows, tile_cols); nnz and ntiles are the caller's (convert.hip)
void set_tiled_shape(pem_tiled *T, int value_bytes, int rows, int cols);
// keys[e] = (tile row | tile column | r << 4 | c) of triplet e, perm[e] = e: the sort key whose order IS the tiled storage order.  n > 0;
// an index outside T's rows x cols raises FLAG_RANGE.  T's shape is the tiling's (already transposed); transpose swaps I and J.
// The head of pem_tiled_from_coo* and of pem_tiled_build* (convert.hip)
void coo_sort_keys(pem_ctx *ctx, const pem_tiled *T, const int *dI, const int *dJ, size_t n, int transpose, int bits_tc, uint64_t *keys,
                   uint32_t *perm);
// sizing phase "tiles" of a tiling whose rows, cols, nnz, ntiles and value_bytes are set: every per-tile array (and the
// nnz-sized payload) in one driver allocation
pem_status reserve_tile_arrays(pem_ctx *ctx, pem_tiled *T);
// reserve_tile_arrays, then the payload derive_tiled starts from (tile_keys, tile_nnz_ptr, vals, rowcolidx) and the tile-head
// scan in ctx->tmp[0], sized by T's nnz and ntiles
pem_status reserve_payload(pem_ctx *ctx, pem_tiled *T);
// where a derived route's payload kernels start: tile_nnz_ptr[0..ntiles] and headx[0] zeroed, ctx->ev[6] recorded;
// *headx = ctx->tmp[0]
pem_status begin_payload(pem_ctx *ctx, pem_tiled *T, int **headx);
// everything that follows from the sorted tile payload (tile_keys, tile_nnz_ptr, rowcolidx, vals); headx[0..nnz] = exclusive
// scan of the tile-head flags.  ctx->ev[6] must have been recorded where the caller's payload kernels start.  Synchronises.
pem_status derive_tiled(pem_ctx *ctx, pem_tiled *T, const int *headx, int bits_tr, int bits_tc);
// headx of a tiling that takes S's pattern as it is (S has entries): the scan straight from S's tile offsets (sddmm.hip; sampled.hip)
void tile_headx(pem_ctx *ctx, const pem_tiled *S, int *headx);
// a derived route's size read-back: the flags (synchronises), then "<fn>: the result's entries exceed the int32 index range"
// where the scan of the counts overflowed or nnz does not fit an int32, then check_internal
pem_status check_result_entries(pem_ctx *ctx, int64_t nnz, const char *fn);
// vmap_t (every entry's slot in vals_t) on first use (values.hip)
pem_status ensure_vmap_t(pem_ctx *ctx, pem_tiled *T);
// vals[e] = vals_t[vmap_t[e]] = src[map[e]], or src[e] where map is null (values.hip).  src holds T's value type; map is
// 16-byte aligned with at least nnz + 4 ints.  vmap_t must be ready.
void refresh_gather(pem_ctx *ctx, pem_tiled *T, const void *src, const int *map);
// the tiling T of S^T from a complete tiling S, by S's column-side arrays (tile CSC, tile_rec_t, vals_t): no entry-level sort
// (chain.hip; pem_tiled_from_cplan(.., 1), pem_tiled_transpose and the column side of pem_tiled_extract).  The caller has zeroed
// the flags and sets T's provenance.  Synchronises.
pem_status transposed_tiling(pem_ctx *ctx, const pem_tiled *S, pem_tiled *T);
// T->derived.map of such a T: every entry's slot in S's vals (int32[nnz + 4]).  Stream-ordered, no read-back (chain.hip).
pem_status build_transpose_map(pem_ctx *ctx, pem_tiled *T);

// ---- the stages of pem_tiled_assign (assign.hip), each the route of its unit with an internal argument ----
// S = A(inv_i, inv_j), rows x cols: extract's gather where an index of -1 is a hole, an output row or column without entries
// (extract.hip).  The lists are device arrays of rows and cols checked values (null: the identity); S gets no provenance.
pem_status scatter_tiling(pem_ctx *ctx, const pem_tiled *A, const int *inv_i, int rows, const int *inv_j, int cols, pem_tiled *S, const char *fn);
// R = C without its entries in the region: select's positional route with the predicate "not (row in I and column in J)"
// (select.hip).  rowbits[P] / colbits[Q]: bit r set where row 16P + r / column 16Q + r is in the list (null: every one is).
pem_status drop_region(pem_ctx *ctx, const pem_tiled *C, const uint16_t *rowbits, const uint16_t *colbits, pem_tiled *R, const char *fn);
// R = the entries of A that a mask stage keeps: select's route around any kernel that writes, per A tile, the new row masks
// (nm: uint32[8T], word q = row 2q | row 2q+1 << 16), the kept count (roff) and a non-empty flag (rid) (select.hip; topk.hip).
// The caller sets R's provenance.  Synchronises.
pem_status select_by_masks(pem_ctx *ctx, const pem_tiled *A, pem_tiled *R, const char *fn,
                           const std::function<void(uint32_t *nm, int *roff, int *rid)> &masks);
// ---- the candidate-tile route (extract.hip; kron.hip, concat.hip): a result built from a list of candidate tiles, 16 lanes each ----
// The read-back after the scan of the candidate counts, whose totals are in ctx->d_scalars[0 .. ntot): the totals into tot, the
// flags (two synchronisations), the unit's own refusal where it has one to make first (refuse(flags): extract's FLAG_RANGE), then
// "<fn>: the result's tiles exceed the int32 index range" on FLAG_OVERFLOW or tot[0] > INT32_MAX, then check_internal.
pem_status check_candidates(pem_ctx *ctx, int ntot, int64_t *tot, const char *fn, const std::function<pem_status(const int *flags)> &refuse = {});
// The launches of a unit on the route: emit writes the ncand candidate keys (tile row << bits_tc) | tile column; count writes per
// candidate its entries and a non-empty flag (a candidate equal to the one before it has none); fill, with the scanned counts
// (roff) and flags (rid), ncand + 1 values each, writes the payload (cand_slots and write_row_bits below).
struct CandidateStages {
    std::function<void(uint64_t *keys)> emit;
    std::function<void(const uint64_t *keys, int *cnt, int *flag)> count;
    std::function<void(const uint64_t *keys, const int *roff, const int *rid, int *headx)> fill;
};
// Everything after ncand is known, on an R whose shape and provenance are set: the keys, their radix sort over R's tile-row and
// tile-column bits (sort), the count, the pair scan and its read-back (check_result_entries; with expect_nnz >= 0 the total must be
// that, or "<fn>: internal: the walk counted %lld entries, not <expect_what> %lld"), R's nnz and ntiles, the payload arrays, the
// fill, derive_tiled.  No stage runs when ncand == 0.  Synchronises: the caller's own temporaries may go once this returns.
pem_status tiling_from_candidates(pem_ctx *ctx, pem_tiled *R, const char *fn, size_t ncand, bool sort, int64_t expect_nnz, const char *expect_what,
                                  const CandidateStages &stages);

// R = op(A, B) over the union of the patterns, alpha = beta = 1: pem_tiled_ewise's build under the caller's name (ewise.hip).
// R's provenance is ewise's; the caller may replace it.
pem_status union_tiling(pem_ctx *ctx, const pem_tiled *A, const pem_tiled *B, int op, pem_tiled *R, const char *fn);
// pem_tiled_set_values_from_ewise's kernel on t's int2 map (t->derived.map) and two value arrays of t's type, alpha = beta = 1
void refresh_pairs(pem_ctx *ctx, pem_tiled *t, const void *a_vals, const void *b_vals, int op);

// The shell of pem_tiled_from_cplan, pem_tiled_ewise and pem_tiled_select (their arguments checked, *out cleared): build(T) into
// a fresh tiling, the time into conv_ms, synchronised; the tiling goes to *out on success and is freed otherwise.
template <typename Build>
pem_status build_derived(pem_ctx *ctx, pem_tiled **out, Build build)
{
    PEM_ENTER(ctx);
    auto t0 = std::chrono::high_resolution_clock::now();
    std::unique_ptr<pem_tiled> T(new pem_tiled());
    pem_status s = build(T.get());
    (void)hipStreamSynchronize(ctx->stream);
    if (s != PEM_OK) return s;
    T->conv_ms = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - t0).count();
    *out = T.release();
    return PEM_OK;
}

// The tail of every pem_tiled_set_values_from_* (arguments and provenance checked): on a tiling with entries, vmap_t and the
// derivation's map on the first call (build_map), then the refresh (launch); value_version bumped.  Stream-ordered, no read-back.
template <typename BuildMap, typename Launch>
pem_status refresh_derived(pem_ctx *ctx, pem_tiled *t, BuildMap build_map, Launch launch)
{
    if (t->nnz) {
        PEM_ENTER(ctx);
        PEM_TRY(ensure_vmap_t(ctx, t));
        if (!t->derived.map_ready) {
            PEM_TRY(build_map());
            t->derived.map_ready = true;
        }
        launch();
    }
    ++t->value_version;
    return PEM_OK;
}

// R's shape, sizes and structural arrays from A: device copies of everything derive_tiled produces but the values; R's vals and
// vals_t (and vmap_t with with_vmap_t) are allocated and left for the caller's kernel (apply.hip; ilu0.hip)
pem_status clone_structure(pem_ctx *ctx, const pem_tiled *A, pem_tiled *R, bool with_vmap_t);

// ---- the level schedule of a triangle (trsv.hip; the lower one is also ILU(0)'s, ilu0.hip) ----
// A->trsv[uplo] on first use: reads the tile CSR back, counts the rows without a stored diagonal entry.  Synchronises once.
pem_status ensure_trsv(pem_ctx *ctx, const pem_tiled *A, int uplo);
// the launches of a schedule under merge width mw: fn(first level, end level, merged) for every one, in order; returns their
// number.  A level wider than mw is one launch, a maximal run of narrower levels is one (merged) launch of one workgroup.
template <typename Fn>
int64_t trsv_for_launches(const TrsvSched &S, int mw, Fn fn)
{
    const int levels = (int)S.h_lvl.size() - 1;
    int64_t launches = 0;
    for (int v = 0; v < levels; ++launches) {
        int e = v + 1;
        const bool merged = S.h_lvl[v + 1] - S.h_lvl[v] <= mw;
        if (merged)
            while (e < levels && S.h_lvl[e + 1] - S.h_lvl[e] <= mw) ++e;
        fn(v, e, merged);
        v = e;
    }
    return launches;
}

// ---- what pem_krylov_create_amg checks of a hierarchy (amg.hip): the context and the operator handle it was created on ----
pem_ctx *amg_owner(const pem_amg *M);
const pem_tiled *amg_operator(const pem_amg *M);

// ---- device: tile lookups in a tiling's tile CSR (mask.hip, ewise.hip; amg.hip) ----
// M's tile id at (i, j), -1 where M has none: binary search in M's tile row i (tile_colidx is sorted inside a row)
__device__ __forceinline__ int mask_find_tile(const int *__restrict__ m_rowptr, const int *__restrict__ m_colidx, const int i, const int j)
{
    int lo = m_rowptr[i];
    const int end = m_rowptr[i + 1];
    int hi = end;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (m_colidx[mid] < j)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < end && m_colidx[lo] == j ? lo : -1;
}

// the first tile of tile row i whose column is >= j (a global tile id; m_rowptr[i + 1] when there is none): where (i, j) is or
// would be in the sorted tile list
__device__ __forceinline__ int tile_lower_bound(const int *__restrict__ m_rowptr, const int *__restrict__ m_colidx, const int i, const int j)
{
    int lo = m_rowptr[i];
    int hi = m_rowptr[i + 1];
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (m_colidx[mid] < j)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// ---- device: one wave per chunk of 64 consecutive tiles, one entry per lane (ewise.hip, select.hip; the search also trsv.hip and line_walk of graph_internal.h) ----
// the wave's LDS writes visible to the whole wave (each wave keeps its own LDS rows: no workgroup barrier)
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the chunk tile (lane) that holds entry e: my_off = the lane's tile's first entry, ascending over the lanes, INT_MAX past the
// chunk's tiles.  A 6-step shuffle search.
__device__ __forceinline__ int chunk_tile_of(const int my_off, const int e)
{
    int ti = 0;
#pragma unroll
    for (int step = 32; step > 0; step >>= 1) {
        const int probe = __shfl(my_off, ti + step, 64);
        if (probe <= e) ti += step;
    }
    return ti;
}

// a tile's row prefixes (entries of the rows above) from its 8 mask words (word q = row 2q | row 2q+1 << 16): row r's prefix in
// byte r & 3 of component r >> 2
__device__ __forceinline__ uint4 row_prefixes(const unsigned w[8])
{
    unsigned rp[4] = {0, 0, 0, 0};
    int run = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        rp[q >> 1] |= (unsigned)run << (16 * (q & 1));
        run += __popc(w[q] & 0xFFFFu);
        rp[q >> 1] |= (unsigned)run << (16 * (q & 1) + 8);
        run += __popc(w[q] >> 16);
    }
    return make_uint4(rp[0], rp[1], rp[2], rp[3]);
}

// the slot in a source tiling's vals of the entry in column c of a row whose tile_rec word is rec (row mask | entries of the
// rows above << 16), in a tile whose first entry is off
__device__ __forceinline__ int src_slot(const int off, const uint32_t rec, const unsigned c)
{
    return off + (int)(rec >> 16) + __popc(rec & ((1u << c) - 1u));
}

// one wave per chunk of 64 consecutive tiles of a tiling R, one entry per lane, the trip count wave-uniform: visit(e, p, q) for
// every entry e of the chunk, (p, q) its row and column in R (long long) from the tile's key and the entry's (r << 4) | c byte.
// The whole body of a refresh-map kernel (extract.hip, assign.hip, kron.hip, concat.hip) but the statement that makes the map word.
template <typename Visit>
__device__ __forceinline__ void for_tile_entries(const long long *__restrict__ r_keys, const long long nt, const int *__restrict__ r_ptr,
                                                 const uint8_t *__restrict__ r_rci, Visit visit)
{
    const int lane = threadIdx.x & 63;
    const long long t0 = (((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6) << 6;
    if (t0 >= nt) return;   // (wave-uniform)
    const int ntl = nt - t0 < 64 ? (int)(nt - t0) : 64;
    const bool live = lane < ntl;
    const long long o = t0 + (live ? lane : 0);
    const int my_off = live ? r_ptr[o] : INT_MAX;
    const int e_end = r_ptr[t0 + ntl];
    const long long key = r_keys[o];
    const int my_tr = (int)(key >> 32), my_tc = (int)(key & 0xFFFFFFFFll);
    const int e_begin = __shfl(my_off, 0, 64);
    for (int ebase = e_begin; ebase < e_end; ebase += 64) {   // wave-uniform trip count
        const int e = ebase + lane;
        const int ti = chunk_tile_of(my_off, e);
        const long long tr = __shfl(my_tr, ti, 64), tc = __shfl(my_tc, ti, 64);
        if (e >= e_end) continue;
        const unsigned rc = r_rci[e];
        visit(e, 16 * tr + (rc >> 4), 16 * tc + (rc & 15u));
    }
}

// ---- device: 16 lanes per candidate result tile, lane = local row r (extract.hip, kron.hip, concat.hip; chain.hip's scatter) ----
// candidate c's tile row and tile column from its key (P << bits_tc) | Q; dup: it equals the key before it (the keys are sorted),
// so it is a duplicate and no tile of its own
struct CandKey {
    long long P, Q;
    bool dup;
};
__device__ __forceinline__ CandKey cand_key(const uint64_t *__restrict__ keys, const long long c, const int bits_tc)
{
    const uint64_t key = keys[c];
    return CandKey{(long long)(key >> bits_tc), (long long)(key & ((1ull << bits_tc) - 1ull)), c > 0 && keys[c - 1] == key};
}

// the end of a count kernel: n = the entries of the lane's row (0 past ncand); cnt[c] = the 16-lane sum, flag[c] = it is not 0.
// Every lane of the group must get here.
__device__ __forceinline__ void cand_count(int n, const long long c, const long long ncand, const int r, int *__restrict__ cnt,
                                           int *__restrict__ flag)
{
#pragma unroll
    for (int d = 8; d > 0; d >>= 1) n += __shfl_xor(n, d, 16);
    if (c < ncand && r == 0) {
        cnt[c] = n;
        flag[c] = n != 0;
    }
}

// the body of a fill kernel: n = the entries of the lane's row (0 past ncand), roff / rid = the scanned counts / flags (ncand + 1
// values each: roff[ncand] = the result's entries, rid[ncand] = its tiles).  Where the candidate is a tile of the result, every
// lane runs fill(s): [s.e0, s.e1) the tile's entries, s.t its id, s.e the row's first slot.  It comes last in the kernel (the
// lanes of a candidate that is no tile have returned, as in a kernel written out), and every lane of the group must get here.
// Nothing of the candidate's key is read: fill decodes it and hands it to cand_tile_head.
struct CandSlots {
    int e, e0, e1, t;
};
template <typename Fill>
__device__ __forceinline__ void cand_slots(const long long c, const long long ncand, const int r, const int n, const int *__restrict__ roff,
                                           const int *__restrict__ rid, int *__restrict__ tile_nnz_ptr, int *__restrict__ headx, Fill fill)
{
    int inc = n;
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) {
        const int v = __shfl_up(inc, d, 16);
        if (r >= d) inc += v;
    }
    if (c == 0 && r == 0) {   // closing offsets: tile_nnz_ptr[T] = nnz, headx[nnz] = T
        const int nt = rid[ncand], nnz = roff[ncand];
        tile_nnz_ptr[nt] = nnz;
        headx[nnz] = nt;
    }
    if (c >= ncand) return;
    const int e0 = roff[c], e1 = roff[c + 1];
    if (e1 == e0) return;
    fill(CandSlots{e0 + (inc - n), e0, e1, rid[c]});
}
// what lane 0 writes of tile s.t: its key from its tile row and tile column, and its first entry
__device__ __forceinline__ void cand_tile_head(const int r, const CandSlots &s, const long long P, const long long Q,
                                               long long *__restrict__ tile_keys, int *__restrict__ tile_nnz_ptr)
{
    if (r == 0) {
        tile_keys[s.t] = (P << 32) | Q;
        tile_nnz_ptr[s.t] = s.e0;
    }
}

// the entries of `bits` (bit b = column place + b of row r of tile `tile`, whose entries are [e0, e_end)) into the payload from slot
// e on: the (r << 4) | c byte, the tile-head scan written directly (tile at the tile's first entry, tile + 1 after it) and the
// value val(b), unless val returns void; returns the slot after them.  val is called once for every bit that is written, in
// ascending order of b, and for no other: a callable may step through a source run (extract.hip).
template <typename VT, typename Val>
__device__ __forceinline__ int write_row_bits(unsigned bits, const unsigned place, const int r, int e, const int e0, const int e_end,
                                              const int tile, uint8_t *__restrict__ rowcolidx, int *__restrict__ headx, VT *__restrict__ vals,
                                              Val val)
{
    while (bits) {
        const unsigned b = (unsigned)__builtin_ctz(bits);
        bits &= bits - 1u;
        if (e < e_end) {   // (the masks and the offsets come from the same counts; never write past the tile)
            rowcolidx[e] = (uint8_t)((r << 4) | (int)(place + b));
            headx[e] = e == e0 ? tile : tile + 1;
            if constexpr (!std::is_void<decltype(val(b))>::value) vals[e] = val(b);
        }
        ++e;
    }
    return e;
}
// rows that carry no values (chain.hip): nothing but the bytes and the tile-head scan is written
__device__ __forceinline__ int write_row_bits(const unsigned bits, const unsigned place, const int r, const int e, const int e0, const int e_end,
                                              const int tile, uint8_t *__restrict__ rowcolidx, int *__restrict__ headx)
{
    return write_row_bits(bits, place, r, e, e0, e_end, tile, rowcolidx, headx, (char *)nullptr, [](unsigned) {});
}

// ---- device: a row of a tiling read as masks, 32 columns at a time (kron.hip, concat.hip) ----
// what such a walk reads of a tiling
struct TileSide {
    const int *rowptr, *colidx;   // tile CSR
    const int *ptr;               // tile_nnz_ptr
    const uint32_t *rec;          // tile_rec: row mask | entries of the rows above << 16
    int rows, cols;
};
inline TileSide tile_side(const pem_tiled *T)
{
    return TileSide{T->tile_rowptr.as<int>(), T->tile_colidx.as<int>(), T->tile_nnz_ptr.as<int>(), T->tile_rec.as<uint32_t>(), T->rows, T->cols};
}

// the 32 columns of row `row` of a tiling that start at tile column tc: the row's masks there (bit b = column 16 tc + b) and, for
// the value slots, the two tiles' tile_rec words and first entries
struct RowSeg {
    uint32_t m, rec0, rec1;
    int off0, off1;
};
__device__ __forceinline__ RowSeg row_seg(const TileSide &S, const int row, const int tc)
{
    const int tr = row >> 4, r = row & 15;
    RowSeg s = {0u, 0u, 0u, 0, 0};
    int t = tile_lower_bound(S.rowptr, S.colidx, tr, tc);
    const int end = S.rowptr[tr + 1];
    if (t < end && S.colidx[t] == tc) {
        s.rec0 = S.rec[16 * (size_t)t + r];
        s.off0 = S.ptr[t];
        ++t;
    }
    if (t < end && S.colidx[t] == tc + 1) {
        s.rec1 = S.rec[16 * (size_t)t + r];
        s.off1 = S.ptr[t];
    }
    s.m = (s.rec0 & 0xFFFFu) | (s.rec1 << 16);
    return s;
}
// the slot in the tiling's vals of the segment's stored column b (0 .. 31)
__device__ __forceinline__ int seg_slot(const RowSeg &s, const unsigned b)
{
    return b < 16u ? src_slot(s.off0, s.rec0, b) : src_slot(s.off1, s.rec1, b - 16u);
}

}  // namespace pem
