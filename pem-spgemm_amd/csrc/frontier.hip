// frontier.hip -- matrix-vector products with a sparse input vector and an output mask (include/pem_spgemm.h,
// pem_tiled_mxv_frontier), and the breadth-first search built on them (pem_tiled_bfs).
//
// x is a dense value array plus one presence byte per entry, y a dense array plus an optional mask byte per output.  The fold of
// every allowed output is mxv's fold (mxv.hip: one wave per line, chunks of 64 entries, regrouped by major in LDS, chained by the
// lane that owns the output) over the stored entries whose x is present -- the plan product A.X with X storing the present x_j --
// and what the presence bytes and the mask rule out is not loaded:
//   pack   one uint16 per 16-entry segment of x: bit b set where x[16 s + b] is present (fr_pack_kernel).  A segment of x is the
//          minor extent of a tile, so a tile whose word is 0 contributes nothing.
//   mark   for every segment with a nonzero word, the tiles of that segment in the OTHER orientation's tile index (tile_colptr /
//          tile_rowidx for A.x, tile_rowptr / tile_colidx for A^T.x) give the lines that can receive anything: line_flag[line] = 1,
//          plain byte stores of one value over a memset (fr_mark_kernel, 16 lanes per segment).
//   walk   frontier_kernel: a wave whose line is not flagged, or none of whose 16 outputs is allowed, writes the start values
//          (accumulate = 0) and the presence zeros and returns before the line's tile index.  Otherwise an entry is live when its
//          tile's word has its minor bit and its major is allowed: only live entries load their value and x, get a slot and are
//          chained; a tile with a zero word does not load its entries' (major, minor) bytes either; a chunk without a live entry
//          does no staging, no sync and no chain.
// With dx_present = NULL there is no pack and no mark: every line is flagged and every word full through the template flag ALLX.
// The words and the flags are the context's (pem_ctx::fr_scratch, grow-only).  No atomics anywhere.
#include "spgemm_internal.h"
#include "tiled_internal.h"
#include "mx_internal.h"
#include <climits>

using namespace pem;

// ------------------------------------------------------------------------------------------
// pack and mark
// ------------------------------------------------------------------------------------------
// one lane per segment; bytes at or beyond nx are never read.  vec: present is 16-byte aligned (whole segments in one load)
__global__ void __launch_bounds__(256) fr_pack_kernel(const uint8_t *__restrict__ present, long long nx, long long nseg, int vec,
                                                      uint16_t *__restrict__ words)
{
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nseg) return;
    const long long b0 = 16 * s;
    unsigned w = 0;
    if (vec && b0 + 16 <= nx) {
        const uint4 q = *reinterpret_cast<const uint4 *>(present + b0);
        const unsigned v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if ((v[i] >> (8 * b)) & 0xFFu) w |= 1u << (4 * i + b);
    } else {
        const int n = (int)(nx - b0 < 16 ? nx - b0 : 16);
        for (int b = 0; b < n; ++b)
            if (present[b0 + b]) w |= 1u << b;
    }
    words[s] = (uint16_t)w;
}

// 16 lanes per segment: sptr[s .. s+1] the segment's tile positions in the other orientation's index, sline[p] the line of the
// tile at position p
__global__ void __launch_bounds__(256) fr_mark_kernel(const uint16_t *__restrict__ words, long long nseg, const int *__restrict__ sptr,
                                                      const int *__restrict__ sline, uint8_t *__restrict__ line_flag, long long nlines)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long s = g >> 4;
    if (s >= nseg || words[s] == 0) return;
    const int p1 = sptr[s + 1];
    for (int p = sptr[s] + (int)(g & 15); p < p1; p += 16) {
        const int L = sline[p];
        if (L >= 0 && L < nlines) line_flag[L] = 1;
    }
}

// ------------------------------------------------------------------------------------------
// the walk (mxv_kernel's, mxv.hip, with the dead entries left out)
// ------------------------------------------------------------------------------------------
// mxv_kernel's arguments, and: words[tile's minor index] the x segment's presence word, line_flag[L] (both unread under ALLX);
// mask / complement: the allowed outputs (null: all); ypres: 1 where an allowed output got a term, else 0 (null: not wanted)
template <typename VT, int K, bool COL, bool ALLX>
__global__ void __launch_bounds__(256) frontier_kernel(const int *__restrict__ lptr, long long nlines, const int *__restrict__ poff,
                                                       const int *__restrict__ pbase, const int *__restrict__ pminor, const uint8_t *__restrict__ rci,
                                                       const VT *__restrict__ vals, const VT *__restrict__ x, const uint16_t *__restrict__ words,
                                                       const uint8_t *__restrict__ line_flag, VT *__restrict__ y, long long nout,
                                                       const uint8_t *__restrict__ mask, int complement, uint8_t *__restrict__ ypres, int accumulate)
{
    using Op = MxOp<K>;
    __shared__ VT s_t[4 * 64];
    __shared__ VT s_x[Op::pair ? 4 * 64 : 1];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long L = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (L >= nlines) return;   // (wave-uniform)
    VT *const my_t = s_t + wv * 64;
    VT *const my_x = s_x + (Op::pair ? wv * 64 : 0);
    const long long o = 16 * L + lane;
    const bool out_lane = lane < 16 && o < nout;
    bool allowed = out_lane;
    if (out_lane && mask) allowed = (mask[o] != 0) != (complement != 0);
    const unsigned allowed_bits = (unsigned)__ballot(allowed);
    bool flagged = true;
    if constexpr (!ALLX) flagged = line_flag[L] != 0;
    if (!flagged || allowed_bits == 0u) {   // (wave-uniform) nothing can enter a fold of this line
        if (allowed && !accumulate) y[o] = Op::template start<VT>();
        if (out_lane && ypres) ypres[o] = 0;
        return;
    }
    VT acc = Op::template start<VT>();
    if (allowed && accumulate) acc = Op::template from_y<VT>(y[o]);
    int touched = 0;
    const int p0 = lptr[L], p1 = lptr[L + 1];
    if (p0 < p1) {
        const int e_end = poff[p1];
        int pc = p0;
        for (int eb = poff[p0]; eb < e_end; eb += 64) {   // wave-uniform trip count
            const int mp = pc + lane;
            const bool lv = mp < p1;
            const int my_off = lv ? poff[mp] : INT_MAX;
            const int my_minor = lv ? pminor[mp] : 0;
            unsigned my_word = 0xFFFFu;
            if constexpr (!ALLX) my_word = lv ? words[my_minor] : 0u;
            int my_base = 0;
            if constexpr (COL) my_base = lv ? pbase[mp] : 0;
            const int e = eb + lane;
            const int ti = chunk_tile_of(my_off, e);
            const int t_off = __shfl(my_off, ti, 64), t_minor = __shfl(my_minor, ti, 64);
            const unsigned t_word = (unsigned)__shfl((int)my_word, ti, 64);
            int t_base = 0;
            if constexpr (COL) t_base = __shfl(my_base, ti, 64);
            const int ti_last = __shfl(ti, 63, 64);
            int major = 16;
            VT a = VT(0), xv = VT(0);
            if (e < e_end && t_word != 0u) {
                const int slot = COL ? t_base + (e - t_off) : e;
                const unsigned rc = rci[slot];
                if (((t_word >> (rc & 15u)) & (allowed_bits >> (rc >> 4)) & 1u) != 0u) {   // live
                    major = (int)(rc >> 4);
                    if constexpr (Op::reads_vals) a = vals[slot];
                    if constexpr (Op::reads_x) xv = x[16 * (size_t)t_minor + (rc & 15u)];
                }
            }
            if (__ballot(major < 16) != 0ull) {   // (wave-uniform) a chunk without a live entry stages and chains nothing
                int slot = 0, my_first = 0, my_cnt = 0, run = 0;
#pragma unroll
                for (int m = 0; m < 16; ++m) {
                    const unsigned long long b = __ballot(major == m);
                    const int n = __popcll(b);
                    if (major == m) slot = run + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
                    if (lane == m) {
                        my_first = run;
                        my_cnt = n;
                    }
                    run += n;
                }
                mx_wave_sync();   // the previous staged chunk's chain has read the staging area
                if (major < 16) {
                    if constexpr (Op::pair) {
                        my_t[slot] = a;
                        my_x[slot] = xv;
                    } else {
                        my_t[slot] = Op::template term<VT>(a, xv);
                    }
                }
                mx_wave_sync();
                touched |= my_cnt;
                const VT *pt = my_t + my_first;
                const VT *px = my_x + (Op::pair ? my_first : 0);
                int k = 0;
                for (; k + 4 <= my_cnt; k += 4) {   // four reads ahead of the chain
                    const VT t0 = pt[k], t1 = pt[k + 1], t2 = pt[k + 2], t3 = pt[k + 3];
                    VT x0 = VT(0), x1 = VT(0), x2 = VT(0), x3 = VT(0);
                    if constexpr (Op::pair) x0 = px[k], x1 = px[k + 1], x2 = px[k + 2], x3 = px[k + 3];
                    acc = Op::template step<VT>(acc, t0, x0);
                    acc = Op::template step<VT>(acc, t1, x1);
                    acc = Op::template step<VT>(acc, t2, x2);
                    acc = Op::template step<VT>(acc, t3, x3);
                }
                for (; k < my_cnt; ++k) acc = Op::template step<VT>(acc, pt[k], Op::pair ? px[k] : VT(0));
            }
            // the next chunk starts in the tile of entry eb + 63, or in the one after it
            int pn = pc + ti_last;
            if (eb + 64 < e_end && pn + 1 < p1 && poff[pn + 1] <= eb + 64) ++pn;
            pc = pn;
        }
    }
    if (allowed && (touched || !accumulate)) y[o] = acc;
    if (out_lane && ypres) ypres[o] = (allowed && touched) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
#define FR_NAMES(vt, k)                                                                                                                  \
    {{"frontier_kernel<" vt "," k ",rows>", "frontier_kernel<" vt "," k ",rows,allx>"},                                                \
     {"frontier_kernel<" vt "," k ",cols>", "frontier_kernel<" vt "," k ",cols,allx>"}}
#define FR_NAMES_VT(vt)                                                                                                                  \
    {FR_NAMES(vt, "plus_times"), FR_NAMES(vt, "min_plus"), FR_NAMES(vt, "max_plus"), FR_NAMES(vt, "max_times"), FR_NAMES(vt, "plus_pair"), \
     FR_NAMES(vt, "lor_land")}
static const char *const kFrNames[2][6][2][2] = {FR_NAMES_VT("float"), FR_NAMES_VT("double")};

pem_status pem::fr_prepare(pem_ctx *ctx, const pem_tiled *A, bool col, const uint8_t *xpres, const uint16_t **words_out, const uint8_t **flags_out)
{
    const long long nx = col ? A->rows : A->cols;
    const long long nlines = col ? A->tile_cols : A->tile_rows;
    const long long nseg = (nx + 15) / 16;   // the other orientation's lines
    ctx->fr_lines = xpres ? nlines : -1;
    *words_out = nullptr;
    *flags_out = nullptr;
    if (col) PEM_TRY(ensure_mx_cols(ctx, A));
    if (!xpres) return PEM_OK;
    const size_t wbytes = ((size_t)nseg * 2 + 255) & ~size_t(255);
    PEM_TRY(ctx->fr_scratch.reserve(wbytes + (size_t)nlines));
    uint16_t *words = ctx->fr_scratch.as<uint16_t>();
    uint8_t *flags = ctx->fr_scratch.as<uint8_t>() + wbytes;
    ctx->fr_flags_off = wbytes;
    PEM_HIP(hipMemsetAsync(flags, 0, (size_t)nlines, ctx->stream));
    if (nseg) {
        const int vec = ((uintptr_t)xpres & 15u) == 0;
        PEM_LAUNCH(ctx, fr_pack_kernel, grid_for((size_t)nseg, 256), 256, xpres, nx, nseg, vec, words);
        if (A->ntiles) {
            if (col)
                PEM_LAUNCH(ctx, fr_mark_kernel, grid_for((size_t)nseg * 16, 256), 256, words, nseg, A->tile_rowptr.as<int>(),
                           A->tile_colidx.as<int>(), flags, nlines);
            else
                PEM_LAUNCH(ctx, fr_mark_kernel, grid_for((size_t)nseg * 16, 256), 256, words, nseg, A->tile_colptr.as<int>(),
                           A->tile_rowidx.as<int>(), flags, nlines);
        }
    }
    *words_out = words;
    *flags_out = flags;
    return PEM_OK;
}

namespace {

struct FrArgs {
    const void *x;
    const uint8_t *xpres;
    void *y;
    const uint8_t *mask;
    int complement;
    uint8_t *ypres;
    int accumulate;
};

template <typename VT, int K, bool COL, bool ALLX>
void fr_launch_walk(pem_ctx *ctx, const pem_tiled *A, const FrArgs &f, const uint16_t *words, const uint8_t *flags)
{
    const char *name = kFrNames[sizeof(VT) == 8][K][COL][ALLX];
    const VT *x = (const VT *)f.x;
    VT *y = (VT *)f.y;
    if constexpr (COL) {
        const long long nlines = A->tile_cols;
        PEM_LAUNCH_NAMED(ctx, name, (frontier_kernel<VT, K, true, ALLX>), grid_for((size_t)nlines * 64, 256), 256, A->tile_colptr.as<int>(), nlines,
                         A->mx_csc_off.as<int>(), A->mx_csc_base.as<int>(), A->tile_rowidx.as<int>(), A->mx_rci_t.as<uint8_t>(),
                         A->vals_t.as<VT>(), x, words, flags, y, (long long)A->cols, f.mask, f.complement, f.ypres, f.accumulate);
    } else {
        const long long nlines = A->tile_rows;
        PEM_LAUNCH_NAMED(ctx, name, (frontier_kernel<VT, K, false, ALLX>), grid_for((size_t)nlines * 64, 256), 256, A->tile_rowptr.as<int>(), nlines,
                         A->tile_nnz_ptr.as<int>(), (const int *)nullptr, A->tile_colidx.as<int>(), A->rowcolidx.as<uint8_t>(),
                         A->vals.as<VT>(), x, words, flags, y, (long long)A->rows, f.mask, f.complement, f.ypres, f.accumulate);
    }
}

template <typename VT, int K>
void fr_launch(pem_ctx *ctx, const pem_tiled *A, bool col, const FrArgs &f, const uint16_t *words, const uint8_t *flags)
{
    if (col) {
        if (f.xpres) fr_launch_walk<VT, K, true, false>(ctx, A, f, words, flags);
        else fr_launch_walk<VT, K, true, true>(ctx, A, f, words, flags);
    } else {
        if (f.xpres) fr_launch_walk<VT, K, false, false>(ctx, A, f, words, flags);
        else fr_launch_walk<VT, K, false, true>(ctx, A, f, words, flags);
    }
}

// the call for checked arguments, inside PEM_ENTER: scratch, pack, mark (fr_prepare), walk.  Stream-ordered, no read-back.
template <typename VT>
pem_status fr_run(pem_ctx *ctx, const pem_tiled *A, int semiring, bool col, const FrArgs &f)
{
    const long long nlines = col ? A->tile_cols : A->tile_rows;
    ctx->fr_lines = f.xpres ? nlines : -1;
    if (nlines == 0) return PEM_OK;   // no output
    const uint16_t *words = nullptr;
    const uint8_t *flags = nullptr;
    PEM_TRY(fr_prepare(ctx, A, col, f.xpres, &words, &flags));
    switch (semiring) {
    case 0: fr_launch<VT, 0>(ctx, A, col, f, words, flags); break;
    case 1: fr_launch<VT, 1>(ctx, A, col, f, words, flags); break;
    case 2: fr_launch<VT, 2>(ctx, A, col, f, words, flags); break;
    case 3: fr_launch<VT, 3>(ctx, A, col, f, words, flags); break;
    case 4: fr_launch<VT, 4>(ctx, A, col, f, words, flags); break;
    default: fr_launch<VT, 5>(ctx, A, col, f, words, flags); break;
    }
    return PEM_OK;
}

pem_status fr_common(pem_ctx *ctx, const pem_tiled *A, int semiring, int transpose, const void *dx, const uint8_t *dx_present, void *dy,
                     const uint8_t *dy_mask, int mask_complement, uint8_t *dy_present, int accumulate, int vb, const char *fn)
{
    if (!ctx || !A) {
        set_error("%s: null context or tiling", fn);
        return PEM_E_INVALID;
    }
    if (semiring < PEM_SEMIRING_PLUS_TIMES || semiring > PEM_SEMIRING_LOR_LAND) {
        set_error("%s: unknown semiring %d (PEM_SEMIRING_PLUS_TIMES .. PEM_SEMIRING_LOR_LAND = 0 .. 5)", fn, semiring);
        return PEM_E_INVALID;
    }
    if (!fr_flag_ok(transpose) || !fr_flag_ok(accumulate) || !fr_flag_ok(mask_complement)) {
        set_error("%s: transpose, accumulate and mask_complement must be 0 or 1 (got %d, %d, %d)", fn, transpose, accumulate, mask_complement);
        return PEM_E_INVALID;
    }
    if (A->value_bytes != vb) {
        set_error("%s: the tiling holds %s values; use the %s entry point", fn, A->value_bytes == 4 ? "fp32" : "fp64",
                  A->value_bytes == 4 ? "_f32" : "fp64");
        return PEM_E_INVALID;
    }
    const bool col = transpose == 1;
    const size_t nx = (size_t)(col ? A->rows : A->cols), ny = (size_t)(col ? A->cols : A->rows);
    if ((semiring != PEM_SEMIRING_PLUS_PAIR && nx && !dx) || (ny && !dy)) {
        set_error("%s: null vector", fn);
        return PEM_E_INVALID;
    }
    const Span sx(dx, nx * vb), sy(dy, ny * vb), sxp(dx_present, nx), sm(dy_mask, ny), syp(dy_present, ny);
    if (sx.meets(sy)) {
        set_error("%s: x and y overlap", fn);
        return PEM_E_INVALID;
    }
    if (syp.meets(sm) || syp.meets(sxp) || syp.meets(sx) || syp.meets(sy)) {
        set_error("%s: dy_present overlaps %s", fn, syp.meets(sm) ? "dy_mask" : syp.meets(sxp) ? "dx_present" : syp.meets(sx) ? "x" : "y");
        return PEM_E_INVALID;
    }
    PEM_ENTER(ctx);
    const FrArgs f{dx, dx_present, dy, dy_mask, mask_complement, dy_present, accumulate};
    return vb == 4 ? fr_run<float>(ctx, A, semiring, col, f) : fr_run<double>(ctx, A, semiring, col, f);
}

}  // namespace

extern "C" pem_status pem_tiled_mxv_frontier(pem_ctx *ctx, const pem_tiled *A, int semiring, int transpose, const double *dx,
                                             const uint8_t *dx_present, double *dy, const uint8_t *dy_mask, int mask_complement,
                                             uint8_t *dy_present, int accumulate)
{
    return fr_common(ctx, A, semiring, transpose, dx, dx_present, dy, dy_mask, mask_complement, dy_present, accumulate, 8, "pem_tiled_mxv_frontier");
}

extern "C" pem_status pem_tiled_mxv_frontier_f32(pem_ctx *ctx, const pem_tiled *A, int semiring, int transpose, const float *dx,
                                                 const uint8_t *dx_present, float *dy, const uint8_t *dy_mask, int mask_complement,
                                                 uint8_t *dy_present, int accumulate)
{
    return fr_common(ctx, A, semiring, transpose, dx, dx_present, dy, dy_mask, mask_complement, dy_present, accumulate, 4,
                     "pem_tiled_mxv_frontier_f32");
}

extern "C" pem_status pem_test_frontier_line_flags(pem_ctx *ctx, uint8_t *host_dst, int64_t nlines)
{
    if (!ctx || (nlines > 0 && !host_dst)) {
        set_error("pem_test_frontier_line_flags: null context or destination");
        return PEM_E_INVALID;
    }
    if (ctx->fr_lines < 0) {
        set_error("pem_test_frontier_line_flags: no frontier call with a dx_present on this context yet, or the last one had none");
        return PEM_E_STATE;
    }
    if (nlines != ctx->fr_lines) {
        set_error("pem_test_frontier_line_flags: the last call had %lld lines, not %lld", (long long)ctx->fr_lines, (long long)nlines);
        return PEM_E_INVALID;
    }
    PEM_ENTER(ctx);
    PEM_TRY(launch_status(ctx));
    if (nlines)
        PEM_HIP(hipMemcpyAsync(host_dst, ctx->fr_scratch.as<uint8_t>() + ctx->fr_flags_off, (size_t)nlines, hipMemcpyDeviceToHost, ctx->stream));
    PEM_HIP(hipStreamSynchronize(ctx->stream));
    return PEM_OK;
}

// ------------------------------------------------------------------------------------------
// breadth-first search
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) bfs_init_kernel(long long n, long long source, int *__restrict__ level, uint8_t *__restrict__ visited,
                                                       uint8_t *__restrict__ frontier)
{
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const bool s = v == source;
    level[v] = s ? 0 : -1;
    visited[v] = s;
    frontier[v] = s;
}

// after a level's product: the new vertices get their level and join visited; found is raised by a plain store of one value
__global__ void __launch_bounds__(256) bfs_level_kernel(long long n, const uint8_t *__restrict__ next, int lvl, int *__restrict__ level,
                                                        uint8_t *__restrict__ visited, int *__restrict__ found)
{
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n || !next[v]) return;
    level[v] = lvl;
    visited[v] = 1;
    *found = 1;
}

// one workgroup: the number of visited vertices
__global__ void __launch_bounds__(1024) bfs_count_kernel(long long n, const uint8_t *__restrict__ visited, long long *__restrict__ out)
{
    __shared__ long long part[16];
    long long c = 0;
    for (long long v = threadIdx.x; v < n; v += 1024) c += visited[v] != 0;
    for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long t = 0;
        for (int w = 0; w < 16; ++w) t += part[w];
        *out = t;
    }
}

extern "C" pem_status pem_tiled_bfs(pem_ctx *ctx, const pem_tiled *A, int64_t source, int transpose, int32_t *d_level, int32_t *depth,
                                    int64_t *reached)
{
    const char *fn = "pem_tiled_bfs";
    if (!ctx || !A || !d_level || !depth || !reached) {
        set_error("%s: null argument", fn);
        return PEM_E_INVALID;
    }
    if (!fr_flag_ok(transpose)) {
        set_error("%s: transpose must be 0 or 1 (got %d)", fn, transpose);
        return PEM_E_INVALID;
    }
    if (A->rows != A->cols) {
        set_error("%s: the tiling is %d x %d; a search needs a square one", fn, A->rows, A->cols);
        return PEM_E_INVALID;
    }
    if (source < 0 || source >= A->rows) {
        set_error("%s: source %lld outside [0, %d)", fn, (long long)source, A->rows);
        return PEM_E_INVALID;
    }
    PEM_ENTER(ctx);
    const long long n = A->rows;
    const size_t nb = ((size_t)n + 255) & ~size_t(255), vb = (size_t)A->value_bytes;
    // visited, two frontiers, the found word and the count, and the product's y (plus_pair's counts: written, never read back)
    DevBuf work;
    PEM_TRY(work.reserve(3 * nb + 256 + (size_t)n * vb));
    uint8_t *visited = work.as<uint8_t>(), *cur = visited + nb, *next = cur + nb;
    int *found = reinterpret_cast<int *>(next + nb);
    long long *count = reinterpret_cast<long long *>(next + nb + 8);
    void *y = next + nb + 256;
    PEM_HIP(hipMemsetAsync(y, 0, (size_t)n * vb, ctx->stream));
    PEM_LAUNCH(ctx, bfs_init_kernel, grid_for((size_t)n, 256), 256, n, (long long)source, d_level, visited, cur);
    int lvl = 0;
    bool any = false;   // the last level found new vertices
    int *const h_found = reinterpret_cast<int *>(ctx->h_scalars);
    for (;;) {
        ++lvl;
        PEM_HIP(hipMemsetAsync(found, 0, sizeof(int), ctx->stream));
        // next = the unvisited ends of the frontier's edges: A^T.f follows them forwards, A.f backwards; accumulate = 1 keeps the
        // lines nothing reaches from writing y
        const FrArgs f{nullptr, cur, y, visited, 1, next, 1};
        PEM_TRY(vb == 4 ? fr_run<float>(ctx, A, PEM_SEMIRING_PLUS_PAIR, transpose == 0, f)
                        : fr_run<double>(ctx, A, PEM_SEMIRING_PLUS_PAIR, transpose == 0, f));
        PEM_LAUNCH(ctx, bfs_level_kernel, grid_for((size_t)n, 256), 256, n, next, lvl, d_level, visited, found);
        PEM_TRY(launch_status(ctx));
        PEM_HIP(hipMemcpyAsync(h_found, found, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        PEM_HIP(hipStreamSynchronize(ctx->stream));
        any = *h_found != 0;
        if (!any || lvl >= n) break;
        uint8_t *t = cur;
        cur = next;
        next = t;
    }
    PEM_LAUNCH(ctx, bfs_count_kernel, 1, 1024, n, visited, count);
    int64_t c = 0;
    PEM_TRY(read_scalars(ctx, reinterpret_cast<const int64_t *>(count), 1, &c));
    PEM_TRY(launch_status(ctx));
    *depth = any ? lvl : lvl - 1;
    *reached = c;
    return PEM_OK;
}
