// ewise.hip -- element-wise combination of two tilings of one shape (include/pem_spgemm.h, pem_tiled_ewise /
// pem_tiled_set_values_from_ewise): R = alpha*A (+) beta*B over the union or the intersection of their patterns.
//
// Both operands are tiled matrices in the same order (tiles by (tile row, tile column), entries row-major inside a tile), so R's
// tiles are a merge of two sorted tile lists and R's entries inside a tile follow from two row masks: no entry-level sort.  The
// route ends, like chain.hip, at the sorted tile payload derive_tiled (convert.hip) starts from:
//   tile matching   one lane per tile of A (and, for the union, per tile of B) binary-searches its (tile row, tile column) in the
//                   other operand's tile row (tile_lower_bound / mask_find_tile, tiled_internal.h) -- a log-time search per tile,
//                   so a tile row holding every tile costs what spread rows cost.
//                     UNION: B's unmatched tiles are flagged and scanned (uscan).  A's tile i lands at i + uscan[its lower bound
//                       in B]; B's unmatched tile j at its lower bound in A + uscan[j].  (a tile's place in the merge is the
//                       number of tiles of either list with a smaller key.)
//                     INTERSECT: A's tiles whose B tile exists and whose ANDed masks are not empty are flagged and scanned.
//                   Every R tile records its A and B source tiles (int2, -1: none) -- kept with R (derived.src_tiles) for the
//                   refresh.
//   counts          one lane per R tile: the 16 row masks ORed or ANDed, popcounted; a scan gives R's entry offsets.
//   payload         one wave per 64 R tiles, one ENTRY per lane (ex_chunkfill_kernel's shape): the tiles' combined masks and row
//                   prefixes in LDS; every entry decodes its tile, row and column and writes its (r<<4|c) byte, the tile-head scan
//                   and its value.  It finds its A and B value slots as step 3 decodes an entry: the source tile's intra-tile row
//                   pointer (tile_rec >> 16) plus the popcount of the row-mask bits below c.  (A first form ran 16 lanes per tile,
//                   lane = row: on webbase-1M's A^2 (+) A it took 1.14 ms, most lanes idle on tiles of a few entries.)
//   derive_tiled    everything else.
// Refresh: the same decode fills an int2 per entry (A slot, B slot, -1: none; derived.map) on the first call; every call is then
// one entry-parallel kernel that gathers both values, applies the op and writes vals and vals_t (through the tiling's vmap_t).
#include "spgemm_internal.h"
#include "tiled_internal.h"

using namespace pem;

// ------------------------------------------------------------------------------------------
// the value rule (header comment of pem_tiled_ewise): scale, then op where both are stored, else the one stored side
// ------------------------------------------------------------------------------------------
struct EwParams {
    int pattern, op;
    double alpha, beta;   // (applied in the value type: (T)alpha * a, skipped when alpha == 1)
};

template <typename VT>
__device__ __forceinline__ VT ew_value(const EwParams &p, bool has_a, VT a, bool has_b, VT b)
{
    if (has_a && p.alpha != 1.0) a = (VT)p.alpha * a;
    if (has_b && p.beta != 1.0) b = (VT)p.beta * b;
    if (!has_b) return a;
    if (!has_a) return b;
    return pem_binop_value<VT>(p.op, a, b);
}

__device__ __forceinline__ unsigned ew_tile_and(const uint16_t *__restrict__ ma, const uint16_t *__restrict__ mb, long long ta, long long tb)
{
    const uint4 *pa = reinterpret_cast<const uint4 *>(ma + 16 * ta), *pb = reinterpret_cast<const uint4 *>(mb + 16 * tb);
    const uint4 a0 = pa[0], a1 = pa[1], b0 = pb[0], b1 = pb[1];
    return (a0.x & b0.x) | (a0.y & b0.y) | (a0.z & b0.z) | (a0.w & b0.w) | (a1.x & b1.x) | (a1.y & b1.y) | (a1.z & b1.z) | (a1.w & b1.w);
}

// ------------------------------------------------------------------------------------------
// tile matching
// ------------------------------------------------------------------------------------------
// UNION, one lane per B tile: unm[j] = B's tile j has no A tile at its position; b_lb[j] = where it would be in A's list
__global__ void ew_bflag_kernel(const long long *__restrict__ b_keys, long long tb, const int *__restrict__ a_rowptr, const int *__restrict__ a_colidx,
                                int *__restrict__ unm, int *__restrict__ b_lb)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= tb) return;
    const long long k = b_keys[j];
    const int i = (int)(k >> 32), c = (int)(k & 0xFFFFFFFFll);
    const int lb = tile_lower_bound(a_rowptr, a_colidx, i, c);
    unm[j] = !(lb < a_rowptr[i + 1] && a_colidx[lb] == c);
    b_lb[j] = lb;
}

// UNION, one lane per tile of A (t < ta) then of B (t - ta): every R tile's sources.  uscan = exclusive scan of unm.
__global__ void ew_place_union_kernel(const long long *__restrict__ a_keys, long long ta, const int *__restrict__ b_rowptr,
                                      const int *__restrict__ b_colidx, long long tb, const int *__restrict__ unm, const int *__restrict__ b_lb,
                                      const int *__restrict__ uscan, int2 *__restrict__ src)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < ta) {
        const long long k = a_keys[t];
        const int i = (int)(k >> 32), c = (int)(k & 0xFFFFFFFFll);
        const int lb = tile_lower_bound(b_rowptr, b_colidx, i, c);
        const bool hit = lb < b_rowptr[i + 1] && b_colidx[lb] == c;
        src[t + uscan[lb]] = make_int2((int)t, hit ? lb : -1);
    } else if (t < ta + tb) {
        const long long j = t - ta;
        if (unm[j]) src[(long long)b_lb[j] + uscan[j]] = make_int2(-1, (int)j);
    }
}

// INTERSECT, one lane per A tile: keep[i] = B holds the tile and the masks meet; b_of[i] = B's tile
__global__ void ew_keep_inter_kernel(const long long *__restrict__ a_keys, long long ta, const int *__restrict__ b_rowptr, const int *__restrict__ b_colidx,
                                     const uint16_t *__restrict__ a_masks, const uint16_t *__restrict__ b_masks, int *__restrict__ keep,
                                     int *__restrict__ b_of)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ta) return;
    const long long k = a_keys[t];
    const int j = mask_find_tile(b_rowptr, b_colidx, (int)(k >> 32), (int)(k & 0xFFFFFFFFll));
    keep[t] = j >= 0 && ew_tile_and(a_masks, b_masks, t, j) != 0u;
    b_of[t] = j;
}

// INTERSECT: kept A tiles to their scanned position (kscan has ta + 1 entries)
__global__ void ew_place_inter_kernel(const int *__restrict__ kscan, const int *__restrict__ b_of, long long ta, int2 *__restrict__ src)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < ta && kscan[t + 1] != kscan[t]) src[kscan[t]] = make_int2((int)t, b_of[t]);
}

// ------------------------------------------------------------------------------------------
// counts and payload
// ------------------------------------------------------------------------------------------
// one lane per R tile: its entry count
__global__ void ew_count_kernel(const int2 *__restrict__ src, long long nt, const uint16_t *__restrict__ a_masks, const uint16_t *__restrict__ b_masks,
                                int inter, int *__restrict__ cnt)
{
    const long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= nt) return;
    const int2 s = src[o];
    int n = 0;
    if (inter) {
        const uint4 *pa = reinterpret_cast<const uint4 *>(a_masks + 16 * (long long)s.x), *pb = reinterpret_cast<const uint4 *>(b_masks + 16 * (long long)s.y);
        const uint4 a0 = pa[0], a1 = pa[1], b0 = pb[0], b1 = pb[1];
        n = __popc(a0.x & b0.x) + __popc(a0.y & b0.y) + __popc(a0.z & b0.z) + __popc(a0.w & b0.w) + __popc(a1.x & b1.x) + __popc(a1.y & b1.y) +
            __popc(a1.z & b1.z) + __popc(a1.w & b1.w);
    } else {
        uint4 a0 = make_uint4(0, 0, 0, 0), a1 = a0, b0 = a0, b1 = a0;
        if (s.x >= 0) {
            const uint4 *pa = reinterpret_cast<const uint4 *>(a_masks + 16 * (long long)s.x);
            a0 = pa[0];
            a1 = pa[1];
        }
        if (s.y >= 0) {
            const uint4 *pb = reinterpret_cast<const uint4 *>(b_masks + 16 * (long long)s.y);
            b0 = pb[0];
            b1 = pb[1];
        }
        n = __popc(a0.x | b0.x) + __popc(a0.y | b0.y) + __popc(a0.z | b0.z) + __popc(a0.w | b0.w) + __popc(a1.x | b1.x) + __popc(a1.y | b1.y) +
            __popc(a1.z | b1.z) + __popc(a1.w | b1.w);
    }
    cnt[o] = n;
}

struct EwSide {
    const long long *keys;
    const int *nnz_ptr;
    const uint32_t *rec;     // tile_rec: row mask | entries of the rows above << 16
    const uint16_t *masks;   // uint16[16T] by row
};

__device__ __forceinline__ void ew_load_masks(const uint16_t *__restrict__ masks, int t, uint4 &m0, uint4 &m1)
{
    if (t < 0) {
        m0 = m1 = make_uint4(0, 0, 0, 0);
        return;
    }
    const uint4 *p = reinterpret_cast<const uint4 *>(masks + 16 * (size_t)t);
    m0 = p[0];
    m1 = p[1];
}

// One wave per chunk of 64 consecutive R tiles, one ENTRY per lane (ex_chunkfill_kernel's shape).  Lane = tile first: R's masks
// (A's and B's ORed or ANDed; word q = row 2q | row 2q+1 << 16, the tiling's layout) and their row prefixes go to LDS, the tile's
// sources and operand offsets stay in the lane's registers.  Then every lane takes one entry of the chunk: its tile by a shuffle
// search over the tiles' offsets, its row by a search over the row prefixes, its column as the k-th set bit of the row's mask, and
// its A and B slots from the source tiles' tile_rec word of that row (intra-tile row pointer + popcount of the mask bits below c).
// ptr = exclusive scan of the counts (ptr[nt] = nnz).  MAP = false: R's payload (tile_keys, tile_nnz_ptr, rowcolidx, headx, vals).
// MAP = true: for R's existing entries, the slots of their operand values in A's and B's vals (-1: none), the refresh's map.
template <typename VT, bool MAP>
__global__ void __launch_bounds__(256) ew_fill_kernel(const int2 *__restrict__ src, long long nt, const int *__restrict__ ptr, EwSide A, EwSide B,
                                                      const VT *__restrict__ a_vals, const VT *__restrict__ b_vals, EwParams prm,
                                                      long long *__restrict__ tile_keys, int *__restrict__ tile_nnz_ptr, uint8_t *__restrict__ rowcolidx,
                                                      int *__restrict__ headx, VT *__restrict__ vals, int2 *__restrict__ map)
{
    __shared__ __attribute__((aligned(16))) uint4 s_rp[4 * 64];   // [wave][tile] prefix counts of the tile's rows, a byte each
    __shared__ unsigned s_mw[4 * 8 * 64];                         // [wave][word q][tile]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long t0 = (((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6) << 6;
    if (!MAP && t0 == 0 && lane == 0) {   // closing offsets: tile_nnz_ptr[T] = nnz, headx[nnz] = T
        const int nnz = ptr[nt];
        tile_nnz_ptr[nt] = nnz;
        headx[nnz] = (int)nt;
    }
    if (t0 >= nt) return;   // (wave-uniform)
    uint4 *const my_rp = s_rp + wv * 64;
    unsigned *const my_mw = s_mw + wv * 512;
    const int ntl = nt - t0 < 64 ? (int)(nt - t0) : 64;
    const bool live = lane < ntl;
    const long long o = t0 + (live ? lane : 0);
    const int2 s = live ? src[o] : make_int2(-1, -1);
    uint4 a0, a1, b0, b1;
    ew_load_masks(A.masks, s.x, a0, a1);
    ew_load_masks(B.masks, s.y, b0, b1);
    unsigned w[8];
    if (prm.pattern == PEM_EWISE_INTERSECT) {
        w[0] = a0.x & b0.x, w[1] = a0.y & b0.y, w[2] = a0.z & b0.z, w[3] = a0.w & b0.w;
        w[4] = a1.x & b1.x, w[5] = a1.y & b1.y, w[6] = a1.z & b1.z, w[7] = a1.w & b1.w;
    } else {
        w[0] = a0.x | b0.x, w[1] = a0.y | b0.y, w[2] = a0.z | b0.z, w[3] = a0.w | b0.w;
        w[4] = a1.x | b1.x, w[5] = a1.y | b1.y, w[6] = a1.z | b1.z, w[7] = a1.w | b1.w;
    }
    const int my_off = live ? ptr[o] : 0x7FFFFFFF;
    const int e_end = ptr[t0 + ntl];
    const int a_off = s.x >= 0 ? A.nnz_ptr[s.x] : 0, b_off = s.y >= 0 ? B.nnz_ptr[s.y] : 0;
    my_rp[lane] = row_prefixes(w);
#pragma unroll
    for (int q = 0; q < 8; ++q) my_mw[q * 64 + lane] = w[q];
    if (!MAP && live) {
        tile_keys[o] = s.x >= 0 ? A.keys[s.x] : B.keys[s.y];
        tile_nnz_ptr[o] = my_off;
    }
    wave_lds_sync();
    const int e_begin = __shfl(my_off, 0, 64);
    for (int ebase = e_begin; ebase < e_end; ebase += 64) {   // wave-uniform trip count
        const int e = ebase + lane;
        const bool valid = e < e_end;
        const int ti = chunk_tile_of(my_off, e);
        const int toff = __shfl(my_off, ti, 64);
        const int sx = __shfl(s.x, ti, 64), sy = __shfl(s.y, ti, 64);
        const int ao = __shfl(a_off, ti, 64), bo = __shfl(b_off, ti, 64);
        if (!valid) continue;
        const unsigned n = (unsigned)(e - toff);
        const uint4 rp4 = my_rp[ti];
        const bool h8 = (rp4.z & 0xFFu) <= n;
        const unsigned d0 = h8 ? rp4.z : rp4.x, d1 = h8 ? rp4.w : rp4.y;
        const bool h4 = (d1 & 0xFFu) <= n;
        const unsigned d = h4 ? d1 : d0;
        const bool h2 = ((d >> 16) & 0xFFu) <= n;
        const unsigned hh = h2 ? d >> 16 : d & 0xFFFFu;
        const bool h1 = ((hh >> 8) & 0xFFu) <= n;
        const int r = (h8 ? 8 : 0) + (h4 ? 4 : 0) + (h2 ? 2 : 0) + (h1 ? 1 : 0);
        const unsigned k0 = n - (h1 ? (hh >> 8) & 0xFFu : hh & 0xFFu);   // rank inside the tile's row r
        const unsigned word = my_mw[(r >> 1) * 64 + ti];
        unsigned m = (r & 1) ? word >> 16 : word & 0xFFFFu, k = k0;
        const unsigned t8 = __popc(m & 0xFFu);
        const bool g8 = k >= t8;
        k -= g8 ? t8 : 0u;
        m = g8 ? m >> 8 : m;
        const unsigned t4 = __popc(m & 0xFu);
        const bool g4 = k >= t4;
        k -= g4 ? t4 : 0u;
        m = g4 ? m >> 4 : m;
        const unsigned t2 = __popc(m & 3u);
        const bool g2 = k >= t2;
        k -= g2 ? t2 : 0u;
        m = g2 ? m >> 2 : m;
        const bool g1 = k >= (m & 1u);
        const int c = (g8 ? 8 : 0) + (g4 ? 4 : 0) + (g2 ? 2 : 0) + (g1 ? 1 : 0);
        const uint32_t wa = sx >= 0 ? A.rec[16 * (size_t)sx + r] : 0u, wb = sy >= 0 ? B.rec[16 * (size_t)sy + r] : 0u;
        const bool ha = (wa >> c) & 1u, hb = (wb >> c) & 1u;
        const int sa = ha ? src_slot(ao, wa, c) : -1;
        const int sb = hb ? src_slot(bo, wb, c) : -1;
        if constexpr (MAP) {
            map[e] = make_int2(sa, sb);
        } else {
            rowcolidx[e] = (uint8_t)((r << 4) | c);
            headx[e] = n == 0 ? (int)(t0 + ti) : (int)(t0 + ti) + 1;
            vals[e] = ew_value<VT>(prm, ha, ha ? a_vals[sa] : VT(0), hb, hb ? b_vals[sb] : VT(0));
        }
    }
}

// refresh: one entry per lane -- both operand values through the map, the op, vals[e] and vals_t[map_t[e]]
template <typename VT>
__global__ void __launch_bounds__(256) ew_refresh_kernel(const int2 *__restrict__ map, const int *__restrict__ map_t, size_t nnz,
                                                         const VT *__restrict__ a_vals, const VT *__restrict__ b_vals, EwParams prm,
                                                         VT *__restrict__ vals, VT *__restrict__ vals_t)
{
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    const int2 s = map[e];
    const bool ha = s.x >= 0, hb = s.y >= 0;
    const VT v = ew_value<VT>(prm, ha, ha ? a_vals[s.x] : VT(0), hb, hb ? b_vals[s.y] : VT(0));
    vals[e] = v;
    vals_t[map_t[e]] = v;
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
static EwSide side_of(const pem_tiled *T)
{
    return EwSide{T->tile_keys.as<long long>(), T->tile_nnz_ptr.as<int>(), T->tile_rec.as<uint32_t>(), T->masks.as<uint16_t>()};
}

static pem_status check_operands(const pem_tiled *A, const pem_tiled *B, const char *fn)
{
    if (A->rows != B->rows || A->cols != B->cols) {
        set_error("%s: A is %d x %d, B is %d x %d", fn, A->rows, A->cols, B->rows, B->cols);
        return PEM_E_INVALID;
    }
    if (A->value_bytes != B->value_bytes) {
        set_error("%s: A holds %s values, B %s", fn, A->value_bytes == 4 ? "fp32" : "fp64", B->value_bytes == 4 ? "fp32" : "fp64");
        return PEM_E_INVALID;
    }
    return PEM_OK;
}

// R's sources per tile into R->derived.src_tiles (int2 per R tile); R->ntiles set
static pem_status match_tiles(pem_ctx *ctx, const pem_tiled *A, const pem_tiled *B, int pattern, pem_tiled *R)
{
    const size_t ta = (size_t)A->ntiles, tb = (size_t)B->ntiles;
    int64_t nt = 0;
    DevBuf src;   // int2 per R tile, sized by the bound ta + tb (union) / ta (intersection); R keeps a copy sized by its tiles
    if (pattern == PEM_EWISE_UNION) {
        DevBuf unm, uscan, b_lb;
        PEM_TRY(unm.reserve(sizeof(int) * (tb + 4)));
        PEM_TRY(uscan.reserve(sizeof(int) * (tb + 4)));
        PEM_TRY(b_lb.reserve(sizeof(int) * (tb + 4)));
        PEM_TRY(src.reserve(sizeof(int2) * (ta + tb + 1)));
        if (tb)
            PEM_LAUNCH(ctx, ew_bflag_kernel, grid_for(tb, 256), 256, B->tile_keys.as<long long>(), (long long)tb, A->tile_rowptr.as<int>(),
                       A->tile_colidx.as<int>(), unm.as<int>(), b_lb.as<int>());
        PEM_TRY(exclusive_scan_i32(ctx, unm.as<int>(), uscan.as<int>(), tb, ctx->d_scalars));
        if (ta + tb)
            PEM_LAUNCH(ctx, ew_place_union_kernel, grid_for(ta + tb, 256), 256, A->tile_keys.as<long long>(), (long long)ta, B->tile_rowptr.as<int>(),
                       B->tile_colidx.as<int>(), (long long)tb, unm.as<int>(), b_lb.as<int>(), uscan.as<int>(), src.as<int2>());
        int64_t nu = 0;
        PEM_TRY(read_scalars(ctx, ctx->d_scalars, 1, &nu));   // (synchronises: the temporaries may go back to the arena)
        nt = (int64_t)ta + nu;
    } else {
        DevBuf keep, b_of;
        PEM_TRY(keep.reserve(sizeof(int) * (ta + 4)));
        PEM_TRY(b_of.reserve(sizeof(int) * (ta + 4)));
        PEM_TRY(src.reserve(sizeof(int2) * (ta + 1)));
        if (ta)
            PEM_LAUNCH(ctx, ew_keep_inter_kernel, grid_for(ta, 256), 256, A->tile_keys.as<long long>(), (long long)ta, B->tile_rowptr.as<int>(),
                       B->tile_colidx.as<int>(), A->masks.as<uint16_t>(), B->masks.as<uint16_t>(), keep.as<int>(), b_of.as<int>());
        PEM_TRY(exclusive_scan_i32(ctx, keep.as<int>(), keep.as<int>(), ta, ctx->d_scalars));
        if (ta) PEM_LAUNCH(ctx, ew_place_inter_kernel, grid_for(ta, 256), 256, keep.as<int>(), b_of.as<int>(), (long long)ta, src.as<int2>());
        PEM_TRY(read_scalars(ctx, ctx->d_scalars, 1, &nt));   // (synchronises)
    }
    int hf[NUM_FLAGS];
    PEM_TRY(read_flags(ctx, hf));
    PEM_TRY(check_internal(hf));
    R->ntiles = nt;
    PEM_TRY(R->derived.src_tiles.reserve(sizeof(int2) * ((size_t)nt + 1)));
    if (nt) PEM_HIP(hipMemcpyAsync(R->derived.src_tiles.p, src.p, sizeof(int2) * (size_t)nt, hipMemcpyDeviceToDevice, ctx->stream));
    return PEM_OK;   // (src goes back to the arena: the copy was enqueued before anything that can reuse it)
}

template <typename VT>
static pem_status ewise_build(pem_ctx *ctx, const pem_tiled *A, const pem_tiled *B, const EwParams &prm, pem_tiled *R, const char *fn)
{
    hipStream_t st = ctx->stream;
    set_tiled_shape(R, A->value_bytes, A->rows, A->cols);
    Derivation &d = R->derived;
    d.kind = Derivation::EWISE;
    d.src[0] = A->serial;
    d.src[1] = B->serial;
    d.pattern = prm.pattern;
    d.op = prm.op;
    d.p0 = prm.alpha;
    d.p1 = prm.beta;
    PEM_TRY(zero_flags(ctx));
    PEM_TRY(match_tiles(ctx, A, B, prm.pattern, R));
    const size_t nt = (size_t)R->ntiles;
    DevBuf ptr;   // int per R tile: entries -> (scanned) R's entry offsets
    PEM_TRY(ptr.reserve(sizeof(int) * (nt + 4)));
    PEM_HIP(hipMemsetAsync(ptr.p, 0, sizeof(int) * (nt + 1), st));
    if (nt)
        PEM_LAUNCH(ctx, ew_count_kernel, grid_for(nt, 256), 256, d.src_tiles.as<int2>(), (long long)nt, A->masks.as<uint16_t>(), B->masks.as<uint16_t>(),
                   prm.pattern == PEM_EWISE_INTERSECT ? 1 : 0, ptr.as<int>());
    PEM_TRY(exclusive_scan_i32(ctx, ptr.as<int>(), ptr.as<int>(), nt, ctx->d_scalars));
    int64_t nnz = 0;
    PEM_TRY(read_scalars(ctx, ctx->d_scalars, 1, &nnz));
    PEM_TRY(check_result_entries(ctx, nnz, fn));
    R->nnz = nnz;
    const int bits_tr = bits_for((uint64_t)R->tile_rows), bits_tc = bits_for((uint64_t)R->tile_cols);
    PEM_TRY(reserve_payload(ctx, R));
    int *headx;
    PEM_TRY(begin_payload(ctx, R, &headx));
    if (nt)
        PEM_LAUNCH(ctx, (ew_fill_kernel<VT, false>), grid_for((nt + 63) / 64 * 64, 256), 256, d.src_tiles.as<int2>(), (long long)nt, ptr.as<int>(), side_of(A),
                   side_of(B), A->vals.as<VT>(), B->vals.as<VT>(), prm, R->tile_keys.as<long long>(), R->tile_nnz_ptr.as<int>(),
                   R->rowcolidx.as<uint8_t>(), headx, R->vals.as<VT>(), nullptr);
    return derive_tiled(ctx, R, headx, bits_tr, bits_tc);
}

static bool params_ok(int pattern, int op, const char *fn)
{
    if (pattern != PEM_EWISE_UNION && pattern != PEM_EWISE_INTERSECT) {
        set_error("%s: pattern %d is neither PEM_EWISE_UNION (0) nor PEM_EWISE_INTERSECT (1)", fn, pattern);
        return false;
    }
    if (op < PEM_BINOP_PLUS || op > PEM_BINOP_LAND) {
        set_error("%s: unknown op %d (PEM_BINOP_PLUS .. PEM_BINOP_LAND = 0 .. 5)", fn, op);
        return false;
    }
    return true;
}

extern "C" pem_status pem_tiled_ewise(pem_ctx *ctx, const pem_tiled *A, const pem_tiled *B, int pattern, int op, double alpha, double beta,
                                      pem_tiled **out)
{
    const char *fn = "pem_tiled_ewise";
    if (!ctx || !A || !B || !out) {
        set_error("%s: null context, operand or output", fn);
        return PEM_E_INVALID;
    }
    *out = nullptr;
    if (!params_ok(pattern, op, fn)) return PEM_E_INVALID;
    PEM_TRY(check_operands(A, B, fn));
    const EwParams prm{pattern, op, alpha, beta};
    return build_derived(ctx, out, [&](pem_tiled *R) {
        return A->value_bytes == 4 ? ewise_build<float>(ctx, A, B, prm, R, fn) : ewise_build<double>(ctx, A, B, prm, R, fn);
    });
}

pem_status pem::union_tiling(pem_ctx *ctx, const pem_tiled *A, const pem_tiled *B, int op, pem_tiled *R, const char *fn)
{
    const EwParams prm{PEM_EWISE_UNION, op, 1.0, 1.0};
    return A->value_bytes == 4 ? ewise_build<float>(ctx, A, B, prm, R, fn) : ewise_build<double>(ctx, A, B, prm, R, fn);
}

static EwParams params_of(const pem_tiled *t)
{
    return EwParams{t->derived.pattern, t->derived.op, t->derived.p0, t->derived.p1};
}

// the decode of the build, once: every entry's operand slots
template <typename VT>
static pem_status ewise_map(pem_ctx *ctx, pem_tiled *t, const pem_tiled *A, const pem_tiled *B)
{
    const size_t nnz = (size_t)t->nnz, nt = (size_t)t->ntiles;
    PEM_TRY(t->derived.map.reserve(sizeof(int2) * (nnz + 1)));
    PEM_LAUNCH(ctx, (ew_fill_kernel<VT, true>), grid_for((nt + 63) / 64 * 64, 256), 256, t->derived.src_tiles.as<int2>(), (long long)nt,
               t->tile_nnz_ptr.as<int>(), side_of(A), side_of(B), A->vals.as<VT>(), B->vals.as<VT>(), params_of(t), nullptr, nullptr, nullptr,
               nullptr, nullptr, t->derived.map.as<int2>());
    return PEM_OK;
}

template <typename VT>
static void ewise_refresh(pem_ctx *ctx, pem_tiled *t, const void *a_vals, const void *b_vals, const EwParams &prm)
{
    const size_t nnz = (size_t)t->nnz;
    PEM_LAUNCH(ctx, ew_refresh_kernel<VT>, grid_for(nnz, 256), 256, t->derived.map.as<int2>(), t->vmap_t.as<int>(), nnz, static_cast<const VT *>(a_vals),
               static_cast<const VT *>(b_vals), prm, t->vals.as<VT>(), t->vals_t.as<VT>());
}

void pem::refresh_pairs(pem_ctx *ctx, pem_tiled *t, const void *a_vals, const void *b_vals, int op)
{
    const EwParams prm{PEM_EWISE_UNION, op, 1.0, 1.0};
    t->value_bytes == 4 ? ewise_refresh<float>(ctx, t, a_vals, b_vals, prm) : ewise_refresh<double>(ctx, t, a_vals, b_vals, prm);
}

extern "C" pem_status pem_tiled_set_values_from_ewise(pem_ctx *ctx, pem_tiled *t, const pem_tiled *A, const pem_tiled *B)
{
    const char *fn = "pem_tiled_set_values_from_ewise";
    if (!ctx || !t || !A || !B) {
        set_error("%s: null context, tiling or operand", fn);
        return PEM_E_INVALID;
    }
    if (t->derived.kind != Derivation::EWISE || t->derived.src[0] != A->serial || t->derived.src[1] != B->serial) {
        set_error("%s: the tiling was not made by pem_tiled_ewise from this A and this B (in this order)", fn);
        return PEM_E_INVALID;
    }
    const bool f32 = t->value_bytes == 4;
    return refresh_derived(
        ctx, t, [&] { return f32 ? ewise_map<float>(ctx, t, A, B) : ewise_map<double>(ctx, t, A, B); },
        [&] { f32 ? ewise_refresh<float>(ctx, t, A->vals.p, B->vals.p, params_of(t)) : ewise_refresh<double>(ctx, t, A->vals.p, B->vals.p, params_of(t)); });
}
