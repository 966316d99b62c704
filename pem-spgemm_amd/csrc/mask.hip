// mask.hip -- masked products C<M> = A*B (pem_cplan_create_masked): the tile filter at the end of step 1.
//
// A masked plan computes only the entries of A*B that the stored pattern of M selects (PEM_MASK_STRUCTURE), or that it does not
// select (PEM_MASK_COMPLEMENT).  Two places make it so, and nothing downstream of them knows about the mask:
//   - here, after step 1 has emitted its sorted pair list, the C tiles are filtered by M's tile set (normal: M holds the tile;
//     complement: M does not hold it, or holds it with fewer than 256 entries) and the pair list, the heads per 256 pairs and
//     _C_rowPtr are compacted to the kept tiles -- step 2 then walks only their pairs;
//   - step 2's s2_tiles_kernel<.., MASKED> ANDs every kept tile's mask with M's tile (or its complement) before it counts and
//     stores it, so the entry counts, the offsets, step 3 and the exports hold C<M>.
// Step 3 keeps its ascending-k fma chain over the same pairs, so a kept entry's value is the unmasked product's bit for bit.
//
// The filter is three passes over the step-1 output, all bandwidth-bound:
//   mask_heads_kernel    one lane per pair; the first pair of every C tile looks (row, column) up in M's sorted tile row and
//                        notes the tile's first pair, M's tile id and whether it is kept
//   mask_count_kernel    one lane per C tile: its pair count where kept (then one scan of both arrays: the kept tiles' and pairs'
//                        new positions, totals = T_C and P of the masked plan)
//   mask_compact_kernel  one lane per pair: kept pairs to their new position (pair_col with its head bit, pairs_a, pairs_b), the
//                        heads per 256 kept pairs (scanned afterwards), M's tile id per kept C tile, _C_rowPtr of the kept tiles
#include "spgemm_internal.h"
#include "tiled_internal.h"

using namespace pem;

__device__ __forceinline__ bool mask_tile_full(const uint16_t *__restrict__ m_masks, const int mt)
{
    const uint4 a = *reinterpret_cast<const uint4 *>(m_masks + 16 * (size_t)mt);
    const uint4 b = *reinterpret_cast<const uint4 *>(m_masks + 16 * (size_t)mt + 8);
    return (a.x & a.y & a.z & a.w & b.x & b.y & b.z & b.w) == 0xFFFFFFFFu;
}

// the C tile of every pair: first pairs in front of its block of 256 (blk_base, scanned) + first pairs in front of it inside the
// block (incl: counting its own).  Lanes of one block; wcnt = the block's shared scratch.
__device__ __forceinline__ long long mask_tile_of(const unsigned long long bal, const int *__restrict__ blk_base, int *wcnt, const bool incl)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wcnt[wave] = __popcll(bal);
    __syncthreads();
    const unsigned long long below = incl ? (2ull << lane) - 1ull : (1ull << lane) - 1ull;
    long long t = (long long)blk_base[blockIdx.x] + __popcll(bal & below);
#pragma unroll
    for (int w = 0; w < 4; ++w)
        if (w < wave) t += wcnt[w];
    return t;
}

__global__ void __launch_bounds__(256) mask_heads_kernel(const int *__restrict__ pair_col, const int *__restrict__ pairs_a, long long npairs,
                                                         const int *__restrict__ blk_base, long long ntc, const long long *__restrict__ a_tile_keys,
                                                         const int *__restrict__ m_rowptr, const int *__restrict__ m_colidx,
                                                         const uint16_t *__restrict__ m_masks, int complement, int *__restrict__ tile_off,
                                                         int *__restrict__ tile_mt, int *__restrict__ keep_t)
{
    __shared__ int wcnt[4];
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    const int col = p < npairs ? pair_col[p] : 0;
    const bool head = col < 0;
    const long long t = mask_tile_of(__ballot(head), blk_base, wcnt, false);
    if (head) {
        const int i = (int)(a_tile_keys[pairs_a[p]] >> 32), j = col & 0x7FFFFFFF;   // (key = tile row << 32 | tile column)
        const int mt = mask_find_tile(m_rowptr, m_colidx, i, j);
        const bool keep = complement ? (mt < 0 || !mask_tile_full(m_masks, mt)) : mt >= 0;
        tile_off[t] = (int)p;
        tile_mt[t] = mt;
        keep_t[t] = keep ? 1 : 0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) tile_off[ntc] = (int)npairs;
}

__global__ void __launch_bounds__(256) mask_count_kernel(const int *__restrict__ tile_off, const int *__restrict__ keep_t, long long ntc,
                                                         int *__restrict__ keep_p)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < ntc) keep_p[t] = keep_t[t] ? tile_off[t + 1] - tile_off[t] : 0;
}

__global__ void __launch_bounds__(256) mask_compact_kernel(const int *__restrict__ pair_col, const int *__restrict__ pairs_a,
                                                           const int *__restrict__ pairs_b, long long npairs, const int *__restrict__ blk_base,
                                                           const int *__restrict__ tile_off, const int *__restrict__ tile_mt,
                                                           const int *__restrict__ keep_t, const int *__restrict__ keep_p,
                                                           int *__restrict__ o_pair_col, int *__restrict__ o_pairs_a, int *__restrict__ o_pairs_b,
                                                           int *__restrict__ o_blk_heads, int *__restrict__ c_mtile, int *__restrict__ c_tile_rowptr,
                                                           int mt)
{
    __shared__ int wcnt[4];
    const int lane = threadIdx.x & 63;
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool valid = p < npairs;
    const int col = valid ? pair_col[p] : 0;
    const bool head = col < 0;
    // (pair 0 is a first pair, so every valid pair has its tile's first pair at or before it: t >= 0)
    const long long t = mask_tile_of(__ballot(head), blk_base, wcnt, true) - 1;
    bool keep = false;
    long long q = 0;
    if (valid) {
        const int k0 = keep_t[t];
        keep = keep_t[t + 1] != k0;
        if (keep) {
            q = (long long)keep_p[t] + (p - tile_off[t]);
            o_pair_col[q] = col;
            o_pairs_a[q] = pairs_a[p];
            o_pairs_b[q] = pairs_b[p];
            if (head) c_mtile[k0] = tile_mt[t];
        }
    }
    // first pairs per 256 kept pairs: the compaction keeps order, so the wave's kept pairs are consecutive in the new list and span
    // at most two blocks of 256
    const unsigned long long K = __ballot(keep), KH = __ballot(keep && head);
    if (KH) {
        const long long b0 = __shfl(q, __builtin_ctzll(K), 64) >> 8;
        const unsigned long long H0 = __ballot(keep && head && (q >> 8) == b0);
        if (lane == 0) {
            const int c0 = __popcll(H0), c1 = __popcll(KH) - c0;
            if (c0) atomicAdd(&o_blk_heads[b0], c0);
            if (c1) atomicAdd(&o_blk_heads[b0 + 1], c1);
        }
    }
    // _C_rowPtr of the kept tiles: kept tiles in front of every tile row's first tile (each entry read and written by one lane)
    for (long long r = p; r <= mt; r += (long long)gridDim.x * 256) c_tile_rowptr[r] = keep_t[c_tile_rowptr[r]];
}

static void swap_buf(DevBuf &a, DevBuf &b)
{
    std::swap(a.p, b.p);
    std::swap(a.cap, b.cap);
    std::swap(a.arena, b.arena);
}

// step 1 of a masked plan writes the same buffers on every pass: the ones the previous pass's filter swapped out
void pem::mask_restore_lists(pem_cplan *p)
{
    if (!p->mf_swapped) return;
    swap_buf(p->pair_col, p->mf_pair_col);
    swap_buf(p->pairs_a, p->mf_pairs_a);
    swap_buf(p->pairs_b, p->mf_pairs_b);
    swap_buf(p->blk_heads, p->mf_blk_heads);
    p->mf_swapped = false;
}

pem_status pem::mask_filter(pem_ctx *ctx, pem_cplan *p, int64_t *P, int64_t *TC)
{
    const pem_tiled *A = p->A, *M = p->M;
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)*P, ntc = (size_t)*TC, nblk = n / 256 + 1;
    const int mt = p->tr_hi - p->tr_lo;
    if (n == 0) {   // nothing to filter; the repeat-pass check still reads the kept counts
        PEM_HIP(hipMemsetAsync(ctx->d_scalars + 4, 0, 2 * sizeof(int64_t), st));
        p->w_Pm = p->w_TCm = 0;
        return PEM_OK;
    }
    PEM_TRY(arena_phase(ctx->arena, {{&p->mf_pair_col, sizeof(int) * (n + 4)}, {&p->mf_pairs_a, sizeof(int) * (n + 4)},
                                     {&p->mf_pairs_b, sizeof(int) * (n + 4)}, {&p->mf_blk_heads, sizeof(int) * (nblk + 4)},
                                     {&p->mf_tile_off, sizeof(int) * (ntc + 4)}, {&p->mf_tile_mt, sizeof(int) * (ntc + 4)},
                                     {&p->mf_keep_t, sizeof(int) * (ntc + 4)}, {&p->mf_keep_p, sizeof(int) * (ntc + 4)},
                                     {&p->c_mtile, sizeof(int) * (ntc + 4)}}));
    PEM_TRY(p->mf_pair_col.reserve(sizeof(int) * (n + 4)));
    PEM_TRY(p->mf_pairs_a.reserve(sizeof(int) * (n + 4)));
    PEM_TRY(p->mf_pairs_b.reserve(sizeof(int) * (n + 4)));
    PEM_TRY(p->mf_blk_heads.reserve(sizeof(int) * (nblk + 4)));
    PEM_TRY(p->mf_tile_off.reserve(sizeof(int) * (ntc + 4)));
    PEM_TRY(p->mf_tile_mt.reserve(sizeof(int) * (ntc + 4)));
    PEM_TRY(p->mf_keep_t.reserve(sizeof(int) * (ntc + 4)));
    PEM_TRY(p->mf_keep_p.reserve(sizeof(int) * (ntc + 4)));
    PEM_TRY(p->c_mtile.reserve(sizeof(int) * (ntc + 4)));
    int *keep_t = p->mf_keep_t.as<int>(), *keep_p = p->mf_keep_p.as<int>();
    const unsigned nb = (unsigned)((n + 255) / 256);
    PEM_LAUNCH(ctx, mask_heads_kernel, nb, 256, p->pair_col.as<int>(), p->pairs_a.as<int>(), (long long)n, p->blk_heads.as<int>(), (long long)ntc,
               A->tile_keys.as<long long>(), M->tile_rowptr.as<int>(), M->tile_colidx.as<int>(), M->masks.as<uint16_t>(), p->mask_complement,
               p->mf_tile_off.as<int>(), p->mf_tile_mt.as<int>(), keep_t);
    PEM_LAUNCH(ctx, mask_count_kernel, grid_for(ntc, 256), 256, p->mf_tile_off.as<int>(), keep_t, (long long)ntc, keep_p);
    // kept tiles / kept pairs in front of every tile; totals: T_C -> d_scalars[5], P -> d_scalars[4]
    PEM_TRY(exclusive_scan_i32_pair(ctx, keep_t, keep_p, ntc, ctx->d_scalars + 5, ctx->d_scalars + 4));
    PEM_HIP(hipMemsetAsync(p->mf_blk_heads.p, 0, sizeof(int) * (nblk + 4), st));
    PEM_LAUNCH(ctx, mask_compact_kernel, nb, 256, p->pair_col.as<int>(), p->pairs_a.as<int>(), p->pairs_b.as<int>(), (long long)n,
               p->blk_heads.as<int>(), p->mf_tile_off.as<int>(), p->mf_tile_mt.as<int>(), keep_t, keep_p, p->mf_pair_col.as<int>(),
               p->mf_pairs_a.as<int>(), p->mf_pairs_b.as<int>(), p->mf_blk_heads.as<int>(), p->c_mtile.as<int>(), p->c_tile_rowptr.as<int>(), mt);
    // (blocks past the kept pairs hold zeros: scanning all nblk keeps the launch the same on every pass)
    PEM_TRY(exclusive_scan_i32(ctx, p->mf_blk_heads.as<int>(), p->mf_blk_heads.as<int>(), nblk, nullptr));
    swap_buf(p->pair_col, p->mf_pair_col);
    swap_buf(p->pairs_a, p->mf_pairs_a);
    swap_buf(p->pairs_b, p->mf_pairs_b);
    swap_buf(p->blk_heads, p->mf_blk_heads);
    p->mf_swapped = true;
    if (p->warm_pass) {
        *P = p->w_Pm;
        *TC = p->w_TCm;
    } else {
        int64_t sc[2];
        PEM_TRY(read_scalars(ctx, ctx->d_scalars + 4, 2, sc));
        *P = p->w_Pm = sc[0];
        *TC = p->w_TCm = sc[1];
    }
    return PEM_OK;
}
