// topk.hip -- the first k entries of every row or column of a tiling in rank order (include/pem_spgemm.h, pem_tiled_select_topk).
//
// R's tiles and entries are a subsequence of A's in A's order, so this is select.hip's route (select_by_masks) around one new mask
// stage: the kernel that decides which entries of a line rank among its first k.  One wave owns one LINE GROUP: a tile row (16
// matrix rows) or, through mxv's column schedule (mx_internal.h), a tile column (16 matrix columns); the 16 lines in it are its
// MAJORS, and every tile belongs to exactly one group, so the wave is the only writer of its tiles' new masks.
//   counts     one walk over the group's TILES: the popcounts of A's row masks (column masks for columns) give every major's entry
//              count n.  A major with n <= k keeps everything.  Where that holds for all 16, the new masks are A's masks and the
//              kept counts the tiles' entry counts: the group is done without having read an entry (the fast path -- the common
//              case of a sparsifying k).
//   pass A     radix select, one threshold per major: every value maps to an unsigned key of its width that descends in rank order
//              (NaN lowest, -0.0 folded onto 0.0, the sign flipped or cleared per order).  From the top 4-bit digit down: the
//              entries whose key still matches their major's prefix are histogrammed into the wave's LDS ([16 digits][16 majors],
//              LDS atomics), lane m scans major m's bins from the top to the digit at which the count reaches what is left of k,
//              narrows the prefix and lowers k.  16 walks of the group for fp64, 8 for fp32, all but the first out of L2.
//   pass B     one more walk: an entry is kept if its key is above its major's threshold, or equals it and is among the first
//              (k - entries above) such entries of its major in walk order -- ascending index inside the line (mxv.hip's header).
//              The tie count of every major lives in lane m and carries across the 64-entry trips and the tiles; inside a trip
//              the rank is a ballot per major plus mbcnt.  Keep bits are ORed into the trip's tiles' masks in LDS; a tile is
//              written (masks, kept count, flag) by one lane once its last entry has passed, and a tile that continues into the
//              next trip carries its words over in LDS.
// No global atomics, nothing depends on wave scheduling: two calls give identical arrays.
#include "spgemm_internal.h"
#include "tiled_internal.h"
#include "mx_internal.h"
#include <climits>

using namespace pem;

// ------------------------------------------------------------------------------------------
// the rank key
// ------------------------------------------------------------------------------------------
// Value bits b of width W -> an unsigned key, larger = earlier in rank order, computed on the bits alone (no arithmetic, so no
// flush of subnormals): a NaN is 0, below every number (the smallest number's key, -inf's, is 0x000F.. / 0x007F.. > 0); both
// zeros become +0; SMALLEST flips the sign, ABS_LARGEST clears it; then the usual monotone map (negative: all bits flipped,
// else the sign bit set).
template <typename U>
__device__ __forceinline__ U tk_key(U b, int order)
{
    constexpr U SIGN = U(1) << (8 * sizeof(U) - 1);
    constexpr U EXPO = (SIGN - 1) & ~((U(1) << (sizeof(U) == 8 ? 52 : 23)) - 1);   // +inf's bits
    const U mag = b & ~SIGN;
    if (mag > EXPO) return U(0);
    if (mag == 0)
        b = 0;
    else if (order == PEM_TOPK_SMALLEST)
        b ^= SIGN;
    else if (order == PEM_TOPK_ABS_LARGEST)
        b = mag;
    return (b & SIGN) ? ~b : (b | SIGN);
}

// ------------------------------------------------------------------------------------------
// the walk: mxv_kernel's, one entry per lane, 64 per trip
// ------------------------------------------------------------------------------------------
// positions p0 .. p1 of the group (p0 < p1); poff[p]: entry offset of position p in walk order (poff[p1] closes the group);
// pbase[p] (COL only): the tile's first slot in vals_t.  f(valid, slot, ti, pc, ti_last, cont) once per trip by the whole wave:
// the lane's entry is valid and sits in slot `slot` of the value array, in the trip's tile ti (position pc + ti); the trip touches
// positions pc .. pc + ti_last, and the last of them continues into the next trip where cont.
template <bool COL, typename F>
__device__ __forceinline__ void tk_walk(const int p0, const int p1, const int *__restrict__ poff, const int *__restrict__ pbase, const int lane, F f)
{
    const int e_end = poff[p1];
    int pc = p0;   // the tile holding the trip's first entry (wave-uniform)
    for (int eb = poff[p0]; eb < e_end; eb += 64) {   // wave-uniform trip count
        const int mp = pc + lane;
        const bool lv = mp < p1;
        const int my_off = lv ? poff[mp] : INT_MAX;
        int my_base = 0;
        if constexpr (COL) my_base = lv ? pbase[mp] : 0;
        const int e = eb + lane;
        const int ti = chunk_tile_of(my_off, e);   // tiles hold 1..256 entries: a trip touches at most 64 of them
        const int t_off = __shfl(my_off, ti, 64);
        int t_base = 0;
        if constexpr (COL) t_base = __shfl(my_base, ti, 64);
        const int ti_last = __shfl(ti, 63, 64);
        const bool valid = e < e_end;
        const int slot = COL ? t_base + (e - t_off) : e;
        // the next trip starts in the tile of entry eb + 63, or in the one after it
        const int pn = pc + ti_last;
        const bool more = eb + 64 < e_end;
        const bool adv = more && pn + 1 < p1 && poff[pn + 1] <= eb + 64;
        f(valid, slot, ti, pc, ti_last, more && !adv);
        pc = adv ? pn + 1 : pn;
    }
}

// ------------------------------------------------------------------------------------------
// the mask stage
// ------------------------------------------------------------------------------------------
// lptr[L .. L+1]: the group's positions; ptile[p] (COL only): the tile at position p (rows: the position is the tile); rci:
// (major << 4) | minor per slot; vals: the value bits per slot; lmasks: uint16[16T], the tiles' masks by major (masks for rows,
// masks_t for columns); masks, tile_nnz_ptr: A's.  k >= 1.  Writes nm, cnt and flag of every tile as sel_band_kernel does.
template <typename U, bool COL>
__global__ void __launch_bounds__(256) topk_mask_kernel(const int *__restrict__ lptr, long long nlines, const int *__restrict__ poff,
                                                        const int *__restrict__ pbase, const int *__restrict__ ptile, const uint8_t *__restrict__ rci,
                                                        const U *__restrict__ vals, const uint16_t *__restrict__ lmasks,
                                                        const uint16_t *__restrict__ masks, const int *__restrict__ tile_nnz_ptr, int order, int k,
                                                        uint32_t *__restrict__ nm, int *__restrict__ cnt, int *__restrict__ flag)
{
    constexpr int BITS = 8 * (int)sizeof(U);
    __shared__ unsigned s_mw[4 * 8 * 64];   // [wave][word q][tile of the trip]
    __shared__ int s_hist[4 * 16 * 16];     // [wave][digit][major]
    __shared__ U s_thr[4 * 16];             // [wave][major]: the prefix (pass A), the threshold key (pass B)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long L = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (L >= nlines) return;   // (wave-uniform)
    const int p0 = lptr[L], p1 = lptr[L + 1];
    if (p0 >= p1) return;
    unsigned *const my_mw = s_mw + wv * 512;
    int *const my_hist = s_hist + wv * 256;
    U *const my_thr = s_thr + wv * 16;

    // counts: lane m < 16 gets major m's entries, from the tiles' masks (64 tiles a trip: 16-bit fields cannot overflow)
    int n_m = 0;
    for (int pb = p0; pb < p1; pb += 64) {   // wave-uniform trip count
        const int p = pb + lane;
        unsigned pk[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (p < p1) {
            const long long t = COL ? ptile[p] : p;
            const uint4 *pm = reinterpret_cast<const uint4 *>(lmasks + 16 * t);
            const uint4 m0 = pm[0], m1 = pm[1];
            const unsigned w[8] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w};
#pragma unroll
            for (int q = 0; q < 8; ++q) pk[q] = (unsigned)__popc(w[q] & 0xFFFFu) | (unsigned)__popc(w[q] >> 16) << 16;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) pk[q] += (unsigned)__shfl_xor((int)pk[q], d, 64);
            if ((lane >> 1) == q) n_m += (int)((pk[q] >> (16 * (lane & 1))) & 0xFFFFu);
        }
    }
    const bool need = lane < 16 && n_m > k;
    const unsigned need_mask = (unsigned)__ballot(need);

    if (need_mask == 0u) {   // no major is cut: the tiles stay as they are
        for (int p = p0 + lane; p < p1; p += 64) {
            const long long t = COL ? ptile[p] : p;
            const uint4 *pm = reinterpret_cast<const uint4 *>(masks + 16 * t);
            uint4 *po = reinterpret_cast<uint4 *>(nm + 8 * t);
            po[0] = pm[0];
            po[1] = pm[1];
            cnt[t] = tile_nnz_ptr[t + 1] - tile_nnz_ptr[t];
            flag[t] = 1;
        }
        return;
    }

    // pass A: the k-th key of every major that is cut, a digit a walk
    U pref = 0;
    int rem = k;   // what is left of k below the entries known to rank above the prefix
    for (int shift = BITS - 4; shift >= 0; shift -= 4) {
#pragma unroll
        for (int i = 0; i < 4; ++i) my_hist[i * 64 + lane] = 0;
        if (lane < 16) my_thr[lane] = pref;
        wave_lds_sync();
        tk_walk<COL>(p0, p1, poff, pbase, lane, [&](bool valid, int slot, int, int, int, bool) {
            if (!valid) return;
            const unsigned major = rci[slot] >> 4;
            if (!((need_mask >> major) & 1u)) return;
            const U key = tk_key<U>(vals[slot], order);
            const int hs = shift + 4;
            if (hs < BITS && ((key ^ my_thr[major]) >> (hs & (BITS - 1))) != 0) return;
            atomicAdd(&my_hist[(int)((key >> shift) & 15u) * 16 + (int)major], 1);
        });
        wave_lds_sync();
        if (need) {
            int run = 0, dsel = 0;
            for (int d = 15; d >= 0; --d) {
                const int c = my_hist[d * 16 + lane];
                if (run + c >= rem) {
                    dsel = d;
                    break;
                }
                run += c;
            }
            pref |= (U)dsel << shift;
            rem -= run;
        }
        wave_lds_sync();
    }

    // pass B: the keep bits.  Lane m holds major m's tie count; a major that is not cut has threshold 0 (a NaN's key) and no limit.
    const int tie_rem = need ? rem : INT_MAX;
    int tie_cnt = 0;
    if (lane < 16) my_thr[lane] = need ? pref : U(0);
#pragma unroll
    for (int q = 0; q < 8; ++q) my_mw[q * 64 + lane] = 0u;
    wave_lds_sync();
    tk_walk<COL>(p0, p1, poff, pbase, lane, [&](bool valid, int slot, int ti, int pc, int ti_last, bool cont) {
        int major = 16;
        bool keep = false, eq = false;
        unsigned word = 0, bit = 0;
        if (valid) {
            const unsigned rc = rci[slot];
            major = (int)(rc >> 4);
            const unsigned minor = rc & 15u;
            const U key = tk_key<U>(vals[slot], order), thr = my_thr[major];
            keep = key > thr;
            eq = key == thr;
            const unsigned r = COL ? minor : (unsigned)major, c = COL ? (unsigned)major : minor;
            word = r >> 1;
            bit = 1u << (c + 16u * (r & 1u));
        }
        if (__ballot(eq) != 0ull) {
#pragma unroll
            for (int m = 0; m < 16; ++m) {
                const unsigned long long b = __ballot(eq && major == m);
                if (b == 0ull) continue;   // (wave-uniform)
                const int base = __shfl(tie_cnt, m, 64), lim = __shfl(tie_rem, m, 64);
                if (eq && major == m) {
                    const int below = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
                    keep = below < lim - base;
                }
                if (lane == m) tie_cnt = base + __popcll(b);
            }
        }
        if (keep) atomicOr(&my_mw[word * 64 + ti], bit);
        wave_lds_sync();
        // the tiles whose last entry has passed, one per lane
        const int nfin = ti_last + 1 - (cont ? 1 : 0);
        if (lane < nfin) {
            const long long t = COL ? ptile[pc + lane] : pc + lane;
            unsigned w[8];
            int n = 0;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                w[q] = my_mw[q * 64 + lane];
                n += __popc(w[q]);
            }
            uint4 *po = reinterpret_cast<uint4 *>(nm + 8 * t);
            po[0] = make_uint4(w[0], w[1], w[2], w[3]);
            po[1] = make_uint4(w[4], w[5], w[6], w[7]);
            cnt[t] = n;
            flag[t] = n != 0;
        }
        // the next trip's staging: empty, but for the words of a tile that continues (it becomes the trip's tile 0)
        unsigned cw[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) cw[q] = (cont && lane == 0) ? my_mw[q * 64 + ti_last] : 0u;
        wave_lds_sync();
#pragma unroll
        for (int q = 0; q < 8; ++q) my_mw[q * 64 + lane] = cw[q];
        wave_lds_sync();
    });
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
template <typename U>
static pem_status topk_build(pem_ctx *ctx, const pem_tiled *A, int order, bool col, int64_t k, pem_tiled *R)
{
    R->derived.kind = Derivation::TOPK;
    R->derived.src[0] = A->serial;
    R->derived.op = order;
    R->derived.pattern = col ? PEM_REDUCE_COLS : PEM_REDUCE_ROWS;
    R->derived.p0 = (double)k;
    const size_t ta = (size_t)A->ntiles;
    const int kk = k > (int64_t)INT_MAX ? INT_MAX : (int)k;   // (a line has fewer than 2^31 entries)
    if (col && ta && kk) PEM_TRY(ensure_mx_cols(ctx, A));
    const char *name = sizeof(U) == 8 ? (col ? "topk_mask_kernel<double,cols>" : "topk_mask_kernel<double,rows>")
                                      : (col ? "topk_mask_kernel<float,cols>" : "topk_mask_kernel<float,rows>");
    return select_by_masks(ctx, A, R, "pem_tiled_select_topk", [&](uint32_t *nm, int *roff, int *rid) {
        if (kk == 0) {   // nothing is kept
            (void)hipMemsetAsync(nm, 0, sizeof(uint32_t) * 8 * ta, ctx->stream);
            (void)hipMemsetAsync(roff, 0, sizeof(int) * ta, ctx->stream);
            (void)hipMemsetAsync(rid, 0, sizeof(int) * ta, ctx->stream);
        } else if (col) {
            const long long nlines = A->tile_cols;
            PEM_LAUNCH_NAMED(ctx, name, (topk_mask_kernel<U, true>), grid_for((size_t)nlines * 64, 256), 256, A->tile_colptr.as<int>(), nlines,
                             A->mx_csc_off.as<int>(), A->mx_csc_base.as<int>(), A->tile_offsets.as<int>(), A->mx_rci_t.as<uint8_t>(),
                             A->vals_t.as<U>(), A->masks_t.as<uint16_t>(), A->masks.as<uint16_t>(), A->tile_nnz_ptr.as<int>(), order, kk, nm, roff,
                             rid);
        } else {
            const long long nlines = A->tile_rows;
            PEM_LAUNCH_NAMED(ctx, name, (topk_mask_kernel<U, false>), grid_for((size_t)nlines * 64, 256), 256, A->tile_rowptr.as<int>(), nlines,
                             A->tile_nnz_ptr.as<int>(), (const int *)nullptr, (const int *)nullptr, A->rowcolidx.as<uint8_t>(), A->vals.as<U>(),
                             A->masks.as<uint16_t>(), A->masks.as<uint16_t>(), A->tile_nnz_ptr.as<int>(), order, kk, nm, roff, rid);
        }
    });
}

extern "C" pem_status pem_tiled_select_topk(pem_ctx *ctx, const pem_tiled *A, int order, int dim, int64_t k, pem_tiled **out)
{
    const char *fn = "pem_tiled_select_topk";
    if (!ctx || !A || !out) {
        set_error("%s: null context, operand or output", fn);
        return PEM_E_INVALID;
    }
    if (order < PEM_TOPK_LARGEST || order > PEM_TOPK_ABS_LARGEST) {
        set_error("%s: unknown order %d (PEM_TOPK_LARGEST, PEM_TOPK_SMALLEST, PEM_TOPK_ABS_LARGEST = 0 .. 2)", fn, order);
        return PEM_E_INVALID;
    }
    if (dim != PEM_REDUCE_ROWS && dim != PEM_REDUCE_COLS) {
        set_error("%s: unknown dim %d (PEM_REDUCE_ROWS = 0, PEM_REDUCE_COLS = 1)", fn, dim);
        return PEM_E_INVALID;
    }
    if (k < 0) {
        set_error("%s: k must be at least 0, not %lld", fn, (long long)k);
        return PEM_E_INVALID;
    }
    *out = nullptr;
    return build_derived(ctx, out, [&](pem_tiled *R) {
        return A->value_bytes == 4 ? topk_build<uint32_t>(ctx, A, order, dim == PEM_REDUCE_COLS, k, R)
                                   : topk_build<uint64_t>(ctx, A, order, dim == PEM_REDUCE_COLS, k, R);
    });
}
