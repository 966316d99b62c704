// select.hip -- entries of a tiling kept by position or by value (include/pem_spgemm.h, pem_tiled_select /
// pem_tiled_set_values_from_select): R holds exactly the stored entries of A that satisfy the predicate, values copied bit for bit.
//
// R's tiles are a subsequence of A's and R's entries a subsequence of A's, both in A's order, so the route needs no sort and no
// search outside a wave.  It ends, like chain.hip and ewise.hip, at the sorted tile payload derive_tiled (convert.hip) starts from:
//   new row masks   positional ops: one lane per A tile ANDs A's 16 row masks with the band rows of the predicate, computed from the
//                   tile's key, the row and k (a tile wholly inside or outside the band gets full or empty band rows; no per-bit
//                   work anywhere).  Value ops: one wave per 64 A tiles, one ENTRY per lane over A's rowcolidx and vals; the keep
//                   bits are ORed into the tiles' masks in LDS.  Either kernel also writes every tile's kept count and a non-empty
//                   flag (one lane per tile popcounts the new masks).
//   scans           one pair scan: the counts give every A tile's entry offset in R, the flags its tile id in R.
//   payload         one wave per 64 A tiles, one ENTRY of A per lane (ew_fill_kernel's shape): the tiles' new masks and row
//                   prefixes in LDS; a kept entry's slot in R is its R tile's offset + the new row prefix + the popcount of the new
//                   row mask below c.  It writes R's tile_keys, tile_nnz_ptr, rowcolidx, tile-head scan and vals, and the A tile
//                   of every R tile (kept with R, derived.src_tiles, for the refresh).
//   derive_tiled    everything else.
// Refresh (positional ops only: their pattern does not depend on A's values): the first call fills an int32 per entry of R, the
// slot of its value in A's vals (one wave per 64 R tiles, the source tile's tile_rec word of the entry's row, as ewise decodes an
// operand slot; derived.map); every call is then values.hip's refresh_gather, four entries per lane, into vals and vals_t.
#include "spgemm_internal.h"
#include "tiled_internal.h"
#include <climits>
#include <cmath>

using namespace pem;

// ------------------------------------------------------------------------------------------
// the predicates (header comment of pem_tiled_select)
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned sel_cols_le(long long d)   // columns c <= d of a row, as a 16-bit mask
{
    return d < 0 ? 0u : d >= 15 ? 0xFFFFu : (2u << d) - 1u;
}

__device__ __forceinline__ unsigned sel_cols_ge(long long d)   // columns c >= d
{
    return d <= 0 ? 0xFFFFu : d > 15 ? 0u : (0xFFFFu << d) & 0xFFFFu;
}

// the columns of matrix row i that the positional op keeps in the tile whose first column is j0 (j = j0 + c)
__device__ __forceinline__ unsigned sel_band_row(int op, long long i, long long j0, long long k)
{
    const long long d = i + k - j0;   // j == i + k  <=>  c == d
    switch (op) {
    case PEM_SELECT_TRIL: return sel_cols_le(d);
    case PEM_SELECT_TRIU: return sel_cols_ge(d);
    case PEM_SELECT_DIAG: return d >= 0 && d <= 15 ? 1u << d : 0u;
    case PEM_SELECT_OFFDIAG: return d >= 0 && d <= 15 ? 0xFFFFu & ~(1u << d) : 0xFFFFu;
    case PEM_SELECT_ROW_LE: return i <= k ? 0xFFFFu : 0u;
    case PEM_SELECT_ROW_GT: return i > k ? 0xFFFFu : 0u;
    case PEM_SELECT_COL_LE: return sel_cols_le(k - j0);
    default: return 0xFFFFu & ~sel_cols_le(k - j0);   // PEM_SELECT_COL_GT
    }
}

// IEEE comparisons in the value type: a NaN x fails all but VALUE_NE; -0.0 == 0.0
template <typename VT>
__device__ __forceinline__ bool sel_keep_value(int op, VT x, VT y)
{
    switch (op) {
    case PEM_SELECT_VALUE_EQ: return x == y;
    case PEM_SELECT_VALUE_NE: return x != y;
    case PEM_SELECT_VALUE_LT: return x < y;
    case PEM_SELECT_VALUE_LE: return x <= y;
    case PEM_SELECT_VALUE_GT: return x > y;
    case PEM_SELECT_VALUE_GE: return x >= y;
    default: return (x < VT(0) ? -x : x) > y;   // PEM_SELECT_ABS_GT (a NaN x stays NaN and fails)
    }
}

// ------------------------------------------------------------------------------------------
// new row masks and counts
// ------------------------------------------------------------------------------------------
// positional ops, one lane per A tile: nm (uint32[8T], word q = row 2q | row 2q+1 << 16, the tiling's layout) = A's masks AND the
// band; cnt[t] its popcount, flag[t] = cnt[t] != 0
__global__ void sel_band_kernel(const long long *__restrict__ keys, const uint16_t *__restrict__ masks, long long ta, int op, long long k,
                                uint32_t *__restrict__ nm, int *__restrict__ cnt, int *__restrict__ flag)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ta) return;
    const long long key = keys[t];
    const long long i0 = 16 * (key >> 32), j0 = 16 * (key & 0xFFFFFFFFll);
    const uint4 *pm = reinterpret_cast<const uint4 *>(masks + 16 * t);
    const uint4 m0 = pm[0], m1 = pm[1];
    unsigned w[8] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w};
    int n = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        w[q] &= sel_band_row(op, i0 + 2 * q, j0, k) | sel_band_row(op, i0 + 2 * q + 1, j0, k) << 16;
        n += __popc(w[q]);
    }
    uint4 *po = reinterpret_cast<uint4 *>(nm + 8 * t);
    po[0] = make_uint4(w[0], w[1], w[2], w[3]);
    po[1] = make_uint4(w[4], w[5], w[6], w[7]);
    cnt[t] = n;
    flag[t] = n != 0;
}

// the region predicate of pem_tiled_assign (drop_region), one lane per A tile like sel_band_kernel: an entry is kept unless its row is
// in I and its column in J.  rowbits[P] / colbits[Q] = the members among tile row P's rows / tile column Q's columns (null: all of
// them), so new mask row r = mask & ~(rowbits[P] >> r & 1 ? colbits[Q] : 0) and a tile wholly outside the region costs one AND.
__global__ void sel_region_kernel(const long long *__restrict__ keys, const uint16_t *__restrict__ masks, long long ta,
                                  const uint16_t *__restrict__ rowbits, const uint16_t *__restrict__ colbits, uint32_t *__restrict__ nm,
                                  int *__restrict__ cnt, int *__restrict__ flag)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ta) return;
    const long long key = keys[t];
    const unsigned rb = rowbits ? rowbits[key >> 32] : 0xFFFFu, cb = colbits ? colbits[key & 0xFFFFFFFFll] : 0xFFFFu;
    const uint4 *pm = reinterpret_cast<const uint4 *>(masks + 16 * t);
    const uint4 m0 = pm[0], m1 = pm[1];
    unsigned w[8] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w};
    int n = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        w[q] &= ~((((rb >> (2 * q)) & 1u) ? cb : 0u) | (((rb >> (2 * q + 1)) & 1u) ? cb << 16 : 0u));
        n += __popc(w[q]);
    }
    uint4 *po = reinterpret_cast<uint4 *>(nm + 8 * t);
    po[0] = make_uint4(w[0], w[1], w[2], w[3]);
    po[1] = make_uint4(w[4], w[5], w[6], w[7]);
    cnt[t] = n;
    flag[t] = n != 0;
}

// value ops: one wave per chunk of 64 consecutive A tiles, one ENTRY per lane.  Lane = tile first: its entry offset stays in the
// lane's register; then every lane takes one entry of the chunk (its tile by a shuffle search over the offsets), tests its value and
// ORs the keep bit into the tile's mask word in LDS.  Lane = tile again: nm, cnt and flag as sel_band_kernel writes them.
template <typename VT>
__global__ void __launch_bounds__(256) sel_value_kernel(const int *__restrict__ a_ptr, const uint8_t *__restrict__ a_rci,
                                                        const VT *__restrict__ a_vals, long long ta, int op, VT y, uint32_t *__restrict__ nm,
                                                        int *__restrict__ cnt, int *__restrict__ flag)
{
    __shared__ unsigned s_mw[4 * 8 * 64];   // [wave][word q][tile]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long t0 = (((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6) << 6;
    if (t0 >= ta) return;   // (wave-uniform)
    unsigned *const my_mw = s_mw + wv * 512;
#pragma unroll
    for (int q = 0; q < 8; ++q) my_mw[q * 64 + lane] = 0u;
    const int ntl = ta - t0 < 64 ? (int)(ta - t0) : 64;
    const bool live = lane < ntl;
    const long long o = t0 + (live ? lane : 0);
    const int my_off = live ? a_ptr[o] : INT_MAX;
    const int e_end = a_ptr[t0 + ntl];
    wave_lds_sync();
    const int e_begin = __shfl(my_off, 0, 64);
    for (int ebase = e_begin; ebase < e_end; ebase += 64) {   // wave-uniform trip count
        const int e = ebase + lane;
        const int ti = chunk_tile_of(my_off, e);
        if (e >= e_end) continue;
        const unsigned rc = a_rci[e];
        if (sel_keep_value<VT>(op, a_vals[e], y)) atomicOr(&my_mw[(rc >> 5) * 64 + ti], 1u << ((rc & 15u) + 16u * ((rc >> 4) & 1u)));
    }
    wave_lds_sync();
    if (!live) return;
    unsigned w[8];
    int n = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        w[q] = my_mw[q * 64 + lane];
        n += __popc(w[q]);
    }
    uint4 *po = reinterpret_cast<uint4 *>(nm + 8 * o);
    po[0] = make_uint4(w[0], w[1], w[2], w[3]);
    po[1] = make_uint4(w[4], w[5], w[6], w[7]);
    cnt[o] = n;
    flag[o] = n != 0;
}

// ------------------------------------------------------------------------------------------
// payload
// ------------------------------------------------------------------------------------------
// One wave per chunk of 64 consecutive A tiles, one ENTRY of A per lane.  Lane = tile first: the tile's new masks and their row
// prefixes go to LDS; its A entry offset, R entry offset (roff, the scanned counts) and R tile id (rid, the scanned flags) stay in
// registers, and a tile that keeps entries writes R's tile_keys, tile_nnz_ptr and src there.  Then every lane takes one entry of
// the chunk: its tile by a shuffle search, its (r, c) from A's rowcolidx; if the new mask holds it, its slot in R is the R tile's
// offset + the new prefix of row r + the popcount of the new row mask below c (the order of A is kept).  roff and rid have ta + 1
// entries (roff[ta] = R's nnz, rid[ta] = R's tiles).
template <typename VT>
__global__ void __launch_bounds__(256) sel_fill_kernel(const long long *__restrict__ a_keys, const int *__restrict__ a_ptr,
                                                       const uint8_t *__restrict__ a_rci, const VT *__restrict__ a_vals, long long ta,
                                                       const uint32_t *__restrict__ nm, const int *__restrict__ roff, const int *__restrict__ rid,
                                                       long long *__restrict__ tile_keys, int *__restrict__ tile_nnz_ptr, int *__restrict__ src,
                                                       uint8_t *__restrict__ rowcolidx, int *__restrict__ headx, VT *__restrict__ vals)
{
    __shared__ __attribute__((aligned(16))) uint4 s_rp[4 * 64];   // [wave][tile] prefix counts of the tile's new rows, a byte each
    __shared__ unsigned s_mw[4 * 8 * 64];                         // [wave][word q][tile]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long t0 = (((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6) << 6;
    if (t0 == 0 && lane == 0) {   // closing offsets: tile_nnz_ptr[T] = nnz, headx[nnz] = T
        const int nnz = roff[ta], nt = rid[ta];
        tile_nnz_ptr[nt] = nnz;
        headx[nnz] = nt;
    }
    if (t0 >= ta) return;   // (wave-uniform)
    uint4 *const my_rp = s_rp + wv * 64;
    unsigned *const my_mw = s_mw + wv * 512;
    const int ntl = ta - t0 < 64 ? (int)(ta - t0) : 64;
    const bool live = lane < ntl;
    const long long o = t0 + (live ? lane : 0);
    unsigned w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (live) {
        const uint4 *p = reinterpret_cast<const uint4 *>(nm + 8 * o);
        const uint4 n0 = p[0], n1 = p[1];
        w[0] = n0.x, w[1] = n0.y, w[2] = n0.z, w[3] = n0.w, w[4] = n1.x, w[5] = n1.y, w[6] = n1.z, w[7] = n1.w;
    }
    const int my_off = live ? a_ptr[o] : INT_MAX;
    const int e_end = a_ptr[t0 + ntl];
    const int r_off = live ? roff[o] : 0, r_id = live ? rid[o] : 0;
    const uint4 rp = row_prefixes(w);
    if (live && (w[0] | w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7]) != 0u) {   // (the tile keeps entries)
        tile_keys[r_id] = a_keys[o];
        tile_nnz_ptr[r_id] = r_off;
        src[r_id] = (int)o;
    }
    my_rp[lane] = rp;
#pragma unroll
    for (int q = 0; q < 8; ++q) my_mw[q * 64 + lane] = w[q];
    wave_lds_sync();
    const int e_begin = __shfl(my_off, 0, 64);
    for (int ebase = e_begin; ebase < e_end; ebase += 64) {   // wave-uniform trip count
        const int e = ebase + lane;
        const int ti = chunk_tile_of(my_off, e);
        const int ro = __shfl(r_off, ti, 64), rd = __shfl(r_id, ti, 64);
        if (e >= e_end) continue;
        const unsigned rc = a_rci[e];
        const unsigned r = rc >> 4, c = rc & 15u;
        const unsigned word = my_mw[(r >> 1) * 64 + ti];
        const unsigned m = (r & 1u) ? word >> 16 : word & 0xFFFFu;
        if (!((m >> c) & 1u)) continue;
        const uint4 rp4 = my_rp[ti];
        const unsigned d = (r >> 2) == 0 ? rp4.x : (r >> 2) == 1 ? rp4.y : (r >> 2) == 2 ? rp4.z : rp4.w;
        const int n = (int)((d >> (8 * (r & 3u))) & 0xFFu) + __popc(m & ((1u << c) - 1u));
        const int slot = ro + n;
        rowcolidx[slot] = (uint8_t)rc;
        headx[slot] = n == 0 ? rd : rd + 1;
        vals[slot] = a_vals[e];
    }
}

// ------------------------------------------------------------------------------------------
// refresh
// ------------------------------------------------------------------------------------------
// the refresh map, once: one wave per chunk of 64 consecutive R tiles, one entry of R per lane; the entry's (r, c) from R's
// rowcolidx, its slot in A's vals from the source tile's tile_rec word of row r (intra-tile row pointer + popcount below c)
__global__ void __launch_bounds__(256) sel_map_kernel(const int *__restrict__ src, long long nt, const int *__restrict__ r_ptr,
                                                      const uint8_t *__restrict__ r_rci, const int *__restrict__ a_ptr,
                                                      const uint32_t *__restrict__ a_rec, int *__restrict__ map)
{
    const int lane = threadIdx.x & 63;
    const long long t0 = (((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6) << 6;
    if (t0 >= nt) return;   // (wave-uniform)
    const int ntl = nt - t0 < 64 ? (int)(nt - t0) : 64;
    const bool live = lane < ntl;
    const long long o = t0 + (live ? lane : 0);
    const int my_off = live ? r_ptr[o] : INT_MAX;
    const int e_end = r_ptr[t0 + ntl];
    const int s = live ? src[o] : 0;
    const int a_off = live ? a_ptr[s] : 0;
    const int e_begin = __shfl(my_off, 0, 64);
    for (int ebase = e_begin; ebase < e_end; ebase += 64) {   // wave-uniform trip count
        const int e = ebase + lane;
        const int ti = chunk_tile_of(my_off, e);
        const int sx = __shfl(s, ti, 64), ao = __shfl(a_off, ti, 64);
        if (e >= e_end) continue;
        const unsigned rc = r_rci[e];
        map[e] = src_slot(ao, a_rec[16 * (size_t)sx + (rc >> 4)], rc & 15u);
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
static bool sel_positional(int op) { return op >= PEM_SELECT_TRIL && op <= PEM_SELECT_COL_GT; }

// the route around its mask kernel: masks(nm, roff, rid) launches the kernel that writes every A tile's new masks, kept count and
// non-empty flag
template <typename VT, typename Masks>
static pem_status select_route(pem_ctx *ctx, const pem_tiled *A, pem_tiled *R, const char *fn, Masks masks)
{
    set_tiled_shape(R, A->value_bytes, A->rows, A->cols);
    const size_t ta = (size_t)A->ntiles;
    PEM_TRY(zero_flags(ctx));
    DevBuf nm, roff, rid;   // per A tile: new masks (uint32[8]); kept count -> R entry offset; non-empty flag -> R tile id
    PEM_TRY(nm.reserve(sizeof(uint32_t) * 8 * (ta + 1)));
    PEM_TRY(roff.reserve(sizeof(int) * (ta + 4)));
    PEM_TRY(rid.reserve(sizeof(int) * (ta + 4)));
    if (ta) masks(nm.as<uint32_t>(), roff.as<int>(), rid.as<int>());
    PEM_TRY(exclusive_scan_i32_pair(ctx, roff.as<int>(), rid.as<int>(), ta, ctx->d_scalars, ctx->d_scalars + 1));
    int64_t tot[2] = {0, 0};
    PEM_TRY(read_scalars(ctx, ctx->d_scalars, 2, tot));
    PEM_TRY(check_result_entries(ctx, tot[0], fn));
    const size_t nnz = (size_t)tot[0], nt = (size_t)tot[1];
    R->nnz = (int64_t)nnz;
    R->ntiles = (int64_t)nt;
    const int bits_tr = bits_for((uint64_t)R->tile_rows), bits_tc = bits_for((uint64_t)R->tile_cols);
    PEM_TRY(reserve_payload(ctx, R));
    PEM_TRY(R->derived.src_tiles.reserve(sizeof(int) * (nt + 1)));
    int *headx;
    PEM_TRY(begin_payload(ctx, R, &headx));
    if (ta)
        PEM_LAUNCH(ctx, sel_fill_kernel<VT>, grid_for((ta + 63) / 64 * 64, 256), 256, A->tile_keys.as<long long>(), A->tile_nnz_ptr.as<int>(),
                   A->rowcolidx.as<uint8_t>(), A->vals.as<VT>(), (long long)ta, nm.as<uint32_t>(), roff.as<int>(), rid.as<int>(),
                   R->tile_keys.as<long long>(), R->tile_nnz_ptr.as<int>(), R->derived.src_tiles.as<int>(), R->rowcolidx.as<uint8_t>(), headx,
                   R->vals.as<VT>());
    return derive_tiled(ctx, R, headx, bits_tr, bits_tc);
}

template <typename VT>
static pem_status select_build(pem_ctx *ctx, const pem_tiled *A, int op, double thunk, pem_tiled *R)
{
    R->derived.kind = Derivation::SELECT;
    R->derived.src[0] = A->serial;
    R->derived.op = op;
    R->derived.p0 = thunk;
    const size_t ta = (size_t)A->ntiles;
    return select_route<VT>(ctx, A, R, "pem_tiled_select", [&](uint32_t *nm, int *roff, int *rid) {
        if (sel_positional(op))
            PEM_LAUNCH(ctx, sel_band_kernel, grid_for(ta, 256), 256, A->tile_keys.as<long long>(), A->masks.as<uint16_t>(), (long long)ta, op,
                       (long long)thunk, nm, roff, rid);
        else
            PEM_LAUNCH(ctx, sel_value_kernel<VT>, grid_for((ta + 63) / 64 * 64, 256), 256, A->tile_nnz_ptr.as<int>(), A->rowcolidx.as<uint8_t>(),
                       A->vals.as<VT>(), (long long)ta, op, (VT)thunk, nm, roff, rid);
    });
}

template <typename VT>
static pem_status region_build(pem_ctx *ctx, const pem_tiled *C, const uint16_t *rowbits, const uint16_t *colbits, pem_tiled *R, const char *fn)
{
    const size_t ta = (size_t)C->ntiles;
    return select_route<VT>(ctx, C, R, fn, [&](uint32_t *nm, int *roff, int *rid) {
        PEM_LAUNCH(ctx, sel_region_kernel, grid_for(ta, 256), 256, C->tile_keys.as<long long>(), C->masks.as<uint16_t>(), (long long)ta, rowbits,
                   colbits, nm, roff, rid);
    });
}

pem_status pem::drop_region(pem_ctx *ctx, const pem_tiled *C, const uint16_t *rowbits, const uint16_t *colbits, pem_tiled *R, const char *fn)
{
    return C->value_bytes == 4 ? region_build<float>(ctx, C, rowbits, colbits, R, fn) : region_build<double>(ctx, C, rowbits, colbits, R, fn);
}

pem_status pem::select_by_masks(pem_ctx *ctx, const pem_tiled *A, pem_tiled *R, const char *fn,
                                const std::function<void(uint32_t *, int *, int *)> &masks)
{
    return A->value_bytes == 4 ? select_route<float>(ctx, A, R, fn, masks) : select_route<double>(ctx, A, R, fn, masks);
}

static bool select_args_ok(int op, double thunk, const char *fn)
{
    if (op < PEM_SELECT_TRIL || op > PEM_SELECT_ABS_GT) {
        set_error("%s: unknown op %d (PEM_SELECT_TRIL .. PEM_SELECT_ABS_GT = 0 .. 14)", fn, op);
        return false;
    }
    if (sel_positional(op) && !(std::floor(thunk) == thunk && std::fabs(thunk) <= 2147483648.0)) {
        set_error("%s: the thunk of a positional op must be an integer k with |k| <= 2^31, not %g", fn, thunk);
        return false;
    }
    return true;
}

extern "C" pem_status pem_tiled_select(pem_ctx *ctx, const pem_tiled *A, int op, double thunk, pem_tiled **out)
{
    const char *fn = "pem_tiled_select";
    if (!ctx || !A || !out) {
        set_error("%s: null context, operand or output", fn);
        return PEM_E_INVALID;
    }
    *out = nullptr;
    if (!select_args_ok(op, thunk, fn)) return PEM_E_INVALID;
    return build_derived(ctx, out, [&](pem_tiled *R) {
        return A->value_bytes == 4 ? select_build<float>(ctx, A, op, thunk, R) : select_build<double>(ctx, A, op, thunk, R);
    });
}

// once: every entry's slot in A's vals (nnz + 4 ints, as refresh_gather's four-entry loads want)
static pem_status select_map(pem_ctx *ctx, pem_tiled *t, const pem_tiled *A)
{
    const size_t nnz = (size_t)t->nnz, nt = (size_t)t->ntiles;
    PEM_TRY(t->derived.map.reserve(sizeof(int) * (nnz + 4)));
    PEM_LAUNCH(ctx, sel_map_kernel, grid_for((nt + 63) / 64 * 64, 256), 256, t->derived.src_tiles.as<int>(), (long long)nt, t->tile_nnz_ptr.as<int>(),
               t->rowcolidx.as<uint8_t>(), A->tile_nnz_ptr.as<int>(), A->tile_rec.as<uint32_t>(), t->derived.map.as<int>());
    return PEM_OK;
}

extern "C" pem_status pem_tiled_set_values_from_select(pem_ctx *ctx, pem_tiled *t, const pem_tiled *A)
{
    const char *fn = "pem_tiled_set_values_from_select";
    if (!ctx || !t || !A) {
        set_error("%s: null context, tiling or source", fn);
        return PEM_E_INVALID;
    }
    if (t->derived.kind != Derivation::SELECT || t->derived.src[0] != A->serial) {
        set_error("%s: the tiling was not made by pem_tiled_select from this A", fn);
        return PEM_E_INVALID;
    }
    if (!sel_positional(t->derived.op)) {
        set_error("%s: the tiling was made by a value predicate (op %d), whose pattern depends on A's values: select again instead", fn,
                  t->derived.op);
        return PEM_E_INVALID;
    }
    return refresh_derived(
        ctx, t, [&] { return select_map(ctx, t, A); }, [&] { refresh_gather(ctx, t, A->vals.p, t->derived.map.as<int>()); });
}
