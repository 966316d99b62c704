// colour.hip -- greedy graph colouring of a square tiling's pattern and the permutation that sorts the vertices by colour
// (include/pem_spgemm.h: pem_tiled_colour, pem_colour_order).
//
// The graph: every stored off-diagonal (i, j) is the undirected edge {i, j}; values are never read.  Every vertex has a priority --
// fmix32(v + seed * 0x9E3779B9) computed in registers, or the caller's d_priority[v] -- larger first, ties to the lower index, and
// colour[v] is the smallest colour no neighbour of higher priority holds: the sequential greedy colouring in that order.  The rounds
// are Jones-Plassmann's, which reproduce it exactly: in a round every uncoloured vertex none of whose uncoloured neighbours beats it
// takes the smallest colour its coloured neighbours leave free.
//   round  colour_round_kernel: the line walk of mxv.hip / frontier.hip -- one wave per line of 16 vertices, chunks of 64 entries,
//          chunk_tile_of, the (major, minor) byte -- over the row line and, unless the caller promised a symmetric pattern, over the
//          column line of the same 16 vertices (the column schedule of mxv.hip).  An entry whose far end is uncoloured and beats the
//          near end raises the near end's bit of the wave's "blocked" word; one whose far end holds a colour in the window
//          [base, base + 64) raises that bit of the near end's 64-bit "used" word.  Both are ORs (LDS atomicOr), so no order shows.
//          A walk stops once every uncoloured vertex of the line is blocked; a vertex whose window is full has the line walked again
//          with the next window (a wave-uniform loop, taken beyond 64 colours only).
//          No kernel reads a colour the same launch writes: a round reads one buffer and writes the other, every line copying its 16
//          colours; a line without an uncoloured vertex returns before its tile index is read.  A wave that leaves a vertex
//          uncoloured raises the round's "more" word by a plain store of one value; the host reads it back (4 bytes per round).
//   order  pem_colour_order: keys = the colours, payload = the vertex numbers, the stable radix sort of primitives.hip on the
//          colours' bits; the offsets are lower bounds in the sorted keys.  A colour outside [0, ncolours) raises FLAG_RANGE and is
//          sorted as colour 0, so every write stays inside its array.
// The scratch of both calls is the context's (pem_ctx::colour_scratch, grow-only).
#include "spgemm_internal.h"
#include "tiled_internal.h"
#include "mx_internal.h"
#include <climits>

using namespace pem;

namespace {

__host__ __device__ __forceinline__ uint32_t fmix32(uint32_t h)
{
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

// what a walk reads of one orientation of a tiling: the arguments of frontier_kernel
struct ColourSide {
    const int *lptr, *poff, *pbase, *pminor;
    const uint8_t *rci;
};

// One orientation's walk for line L.  want: the vertices (bits) of the line whose neighbours matter; first: the pass that also tests
// the priorities (later windows only collect colours: their vertices are known to be unblocked).  my_prio: lane m < 16 holds the
// priority of vertex 16 L + m.  Returns true when every wanted vertex is blocked (first pass only): nothing more can change.
template <bool COL, bool HASH>
__device__ __forceinline__ bool colour_walk(const ColourSide &S, const long long L, const int lane, const unsigned want, const bool first,
                                            const uint32_t my_prio, const uint32_t seed_term, const uint32_t *__restrict__ prio,
                                            const int *__restrict__ colour_in, const int base, unsigned long long *used, unsigned *blk)
{
    const int p0 = S.lptr[L], p1 = S.lptr[L + 1];
    if (p0 >= p1) return false;
    const int e_end = S.poff[p1];
    int pc = p0;
    for (int eb = S.poff[p0]; eb < e_end; eb += 64) {   // wave-uniform trip count
        const int mp = pc + lane;
        const bool lv = mp < p1;
        const int my_off = lv ? S.poff[mp] : INT_MAX;
        const int my_minor = lv ? S.pminor[mp] : 0;
        int my_base = 0;
        if constexpr (COL) my_base = lv ? S.pbase[mp] : 0;
        const int e = eb + lane;
        const int ti = chunk_tile_of(my_off, e);
        const int t_off = __shfl(my_off, ti, 64), t_minor = __shfl(my_minor, ti, 64);
        int t_base = 0;
        if constexpr (COL) t_base = __shfl(my_base, ti, 64);
        const int ti_last = __shfl(ti, 63, 64);
        const bool in = e < e_end;
        unsigned rc = 0;
        if (in) rc = S.rci[COL ? t_base + (e - t_off) : e];
        const unsigned major = rc >> 4;
        const uint32_t pi = (uint32_t)__shfl((int)my_prio, (int)major, 64);
        const long long i = 16 * L + major, j = 16 * (long long)t_minor + (rc & 15u);
        if (in && ((want >> major) & 1u) != 0u && j != i) {
            const int cj = colour_in[j];
            if (cj < 0) {
                if (first) {
                    const uint32_t pj = HASH ? fmix32((uint32_t)j + seed_term) : prio[j];
                    if (pj > pi || (pj == pi && j < i)) atomicOr(blk, 1u << major);
                }
            } else if (cj >= base && cj - base < 64) {
                atomicOr(&used[major], 1ull << (cj - base));
            }
        }
        if (first) {
            mx_wave_sync();
            if ((__builtin_amdgcn_readfirstlane(*blk) & want) == want) return true;   // (wave-uniform)
        }
        // the next chunk starts in the tile of entry eb + 63, or in the one after it
        int pn = pc + ti_last;
        if (eb + 64 < e_end && pn + 1 < p1 && S.poff[pn + 1] <= eb + 64) ++pn;
        pc = pn;
    }
    return false;
}

// one round: colour_out = colour_in with every unblocked uncoloured vertex coloured.  *more is raised where a vertex stays
// uncoloured; *more_next, the next round's word, is cleared (nobody else touches it in this launch).
template <bool SYM, bool HASH>
__global__ void __launch_bounds__(256) colour_round_kernel(const ColourSide R, const ColourSide Cs, const long long nlines, const long long n,
                                                           const uint32_t seed_term, const uint32_t *__restrict__ prio,
                                                           const int *__restrict__ colour_in, int *__restrict__ colour_out, int *more, int *more_next)
{
    __shared__ unsigned long long s_used[4 * 16];
    __shared__ unsigned s_blk[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long L = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (blockIdx.x == 0 && threadIdx.x == 0) *more_next = 0;
    if (L >= nlines) return;   // (wave-uniform)
    const long long v = 16 * L + lane;
    const bool mine = lane < 16 && v < n;
    int c = mine ? colour_in[v] : 0;
    unsigned want = (unsigned)__ballot(mine && c < 0);
    if (want == 0u) {   // (wave-uniform) nothing left to colour in this line
        if (mine) colour_out[v] = c;
        return;
    }
    unsigned long long *const used = s_used + wv * 16;
    unsigned *const blk = s_blk + wv;
    uint32_t my_prio = 0;
    if (mine) my_prio = HASH ? fmix32((uint32_t)v + seed_term) : prio[v];
    if (lane < 16) used[lane] = 0ull;
    if (lane == 0) *blk = 0u;
    mx_wave_sync();
    bool first = true;
    for (int base = 0; want != 0u; base += 64) {   // (wave-uniform) one trip per window of 64 colours
        bool all_blocked = colour_walk<false, HASH>(R, L, lane, want, first, my_prio, seed_term, prio, colour_in, base, used, blk);
        if constexpr (!SYM)
            if (!all_blocked) all_blocked = colour_walk<true, HASH>(Cs, L, lane, want, first, my_prio, seed_term, prio, colour_in, base, used, blk);
        if (all_blocked) break;
        mx_wave_sync();
        bool full = false;
        if (lane < 16 && ((want >> lane) & 1u) != 0u && ((*blk >> lane) & 1u) == 0u) {
            const unsigned long long free_bits = ~used[lane];
            if (free_bits != 0ull)
                c = base + __ffsll((long long)free_bits) - 1;
            else
                full = true;
        }
        want = (unsigned)__ballot(full);
        first = false;
        mx_wave_sync();   // every lane has read its word
        if (lane < 16) used[lane] = 0ull;
        mx_wave_sync();
    }
    if (mine) colour_out[v] = c;
    if (__ballot(mine && c < 0) != 0ull && lane == 0) *more = 1;
}

// one block's largest colour into *out (started at -1)
__global__ void __launch_bounds__(256) colour_max_kernel(const int *__restrict__ colour, const long long n, int *__restrict__ out)
{
    __shared__ int part[4];
    int m = -1;
    for (long long v = (long long)blockIdx.x * 1024 + threadIdx.x, k = 0; k < 4 && v < n; ++k, v += 256) m = max(m, colour[v]);
    for (int d = 32; d > 0; d >>= 1) m = max(m, __shfl_down(m, d, 64));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = max(max(part[0], part[1]), max(part[2], part[3]));
        if (m >= 0) atomicMax(out, m);
    }
}

// ---- the colour order ----
__global__ void __launch_bounds__(256) order_keys_kernel(const int *__restrict__ colour, const long long n, const int ncolours,
                                                         uint64_t *__restrict__ keys, uint32_t *__restrict__ verts, int *__restrict__ flags)
{
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    int c = colour[v];
    if (c < 0 || c >= ncolours) {
        flags[FLAG_RANGE] = 1;
        c = 0;
    }
    keys[v] = (uint64_t)c;
    verts[v] = (uint32_t)v;
}

// perm = the sorted vertices; offsets[c] = the first position whose colour is >= c
__global__ void __launch_bounds__(256) order_finish_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ verts, const long long n,
                                                           const int ncolours, int *__restrict__ perm, int *__restrict__ offsets)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) perm[t] = (int)verts[t];
    if (t <= ncolours) {
        long long lo = 0, hi = n;
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (keys[mid] < (uint64_t)t)
                lo = mid + 1;
            else
                hi = mid;
        }
        offsets[t] = (int)lo;
    }
}

template <bool SYM>
void colour_launch(pem_ctx *ctx, bool hash, const ColourSide &R, const ColourSide &Cs, long long nlines, long long n, uint32_t seed_term,
                   const uint32_t *prio, const int *cin, int *cout, int *more, int *more_next)
{
    const unsigned grid = grid_for((size_t)nlines * 64, 256);
    if (hash)
        PEM_LAUNCH_NAMED(ctx, SYM ? "colour_round_kernel<rows,hash>" : "colour_round_kernel<both,hash>", (colour_round_kernel<SYM, true>), grid, 256,
                         R, Cs, nlines, n, seed_term, prio, cin, cout, more, more_next);
    else
        PEM_LAUNCH_NAMED(ctx, SYM ? "colour_round_kernel<rows,priority>" : "colour_round_kernel<both,priority>",
                         (colour_round_kernel<SYM, false>), grid, 256, R, Cs, nlines, n, seed_term, prio, cin, cout, more, more_next);
}

}  // namespace

extern "C" pem_status pem_tiled_colour(pem_ctx *ctx, const pem_tiled *A, int symmetric, uint32_t seed, const uint32_t *d_priority,
                                       int32_t *d_colour, int32_t *ncolours, int32_t *rounds)
{
    const char *fn = "pem_tiled_colour";
    if (!ctx || !A || !d_colour || !ncolours || !rounds) {
        set_error("%s: null argument", fn);
        return PEM_E_INVALID;
    }
    if (A->rows != A->cols) {
        set_error("%s: the tiling is %d x %d; a colouring needs a square one", fn, A->rows, A->cols);
        return PEM_E_INVALID;
    }
    if (!fr_flag_ok(symmetric)) {
        set_error("%s: symmetric must be 0 or 1 (got %d)", fn, symmetric);
        return PEM_E_INVALID;
    }
    const long long n = A->rows;
    if (Span(d_priority, (size_t)n * 4).meets(Span(d_colour, (size_t)n * 4))) {
        set_error("%s: d_priority and d_colour overlap", fn);
        return PEM_E_INVALID;
    }
    *ncolours = 0;
    *rounds = 0;
    if (n == 0) return PEM_OK;
    PEM_ENTER(ctx);
    if (!symmetric) PEM_TRY(ensure_mx_cols(ctx, A));
    // the second colour buffer, then the two "more" words and the largest colour
    const size_t cbytes = ((size_t)n * sizeof(int) + 255) & ~size_t(255);
    PEM_TRY(ctx->colour_scratch.reserve(cbytes + 256));
    int *buf[2] = {d_colour, ctx->colour_scratch.as<int>()};
    int *const words = reinterpret_cast<int *>(ctx->colour_scratch.as<char>() + cbytes);   // more[2], then the largest colour
    const ColourSide R{A->tile_rowptr.as<int>(), A->tile_nnz_ptr.as<int>(), nullptr, A->tile_colidx.as<int>(), A->rowcolidx.as<uint8_t>()};
    const ColourSide Cs{A->tile_colptr.as<int>(), A->mx_csc_off.as<int>(), A->mx_csc_base.as<int>(), A->tile_rowidx.as<int>(),
                        A->mx_rci_t.as<uint8_t>()};
    const long long nlines = A->tile_rows;
    const uint32_t seed_term = seed * 0x9E3779B9u;
    PEM_HIP(hipMemsetAsync(buf[0], 0xFF, (size_t)n * sizeof(int), ctx->stream));   // every vertex uncoloured (-1)
    PEM_HIP(hipMemsetAsync(words, 0, 2 * sizeof(int), ctx->stream));
    PEM_HIP(hipMemsetAsync(words + 2, 0xFF, sizeof(int), ctx->stream));
    int *const h_more = reinterpret_cast<int *>(ctx->h_scalars);
    int r = 0;
    for (;;) {   // round r + 1 reads buf[r & 1], writes the other, raises words[r & 1] and clears the other word
        int *const more = words + (r & 1), *const more_next = words + ((r + 1) & 1);
        if (symmetric)
            colour_launch<true>(ctx, d_priority == nullptr, R, Cs, nlines, n, seed_term, d_priority, buf[r & 1], buf[(r + 1) & 1], more, more_next);
        else
            colour_launch<false>(ctx, d_priority == nullptr, R, Cs, nlines, n, seed_term, d_priority, buf[r & 1], buf[(r + 1) & 1], more, more_next);
        PEM_TRY(launch_status(ctx));
        PEM_HIP(hipMemcpyAsync(h_more, more, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        PEM_HIP(hipStreamSynchronize(ctx->stream));
        ++r;
        if (*h_more == 0) break;
        if (r >= n) {   // (every round colours the best uncoloured vertex at least)
            set_error("%s: internal: vertices left uncoloured after %d rounds", fn, r);
            return PEM_E_HIP;
        }
    }
    if (r & 1) PEM_HIP(hipMemcpyAsync(d_colour, buf[1], (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, ctx->stream));
    PEM_LAUNCH(ctx, colour_max_kernel, grid_for((size_t)n, 1024), 256, d_colour, n, words + 2);
    PEM_TRY(launch_status(ctx));
    PEM_HIP(hipMemcpyAsync(h_more, words + 2, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    PEM_HIP(hipStreamSynchronize(ctx->stream));
    *ncolours = *h_more + 1;
    *rounds = r;
    return PEM_OK;
}

extern "C" pem_status pem_colour_order(pem_ctx *ctx, int64_t n, const int32_t *d_colour, int32_t ncolours, int32_t *d_perm, int32_t *d_offsets)
{
    const char *fn = "pem_colour_order";
    if (!ctx || !d_colour || !d_perm || !d_offsets) {
        set_error("%s: null argument", fn);
        return PEM_E_INVALID;
    }
    if (n < 0 || n > INT32_MAX || ncolours < 0 || (ncolours == 0 && n > 0)) {
        set_error("%s: n = %lld, ncolours = %d: want 0 <= n <= INT32_MAX and ncolours >= 0, at least 1 where n > 0", fn, (long long)n, ncolours);
        return PEM_E_INVALID;
    }
    const Span sc(d_colour, (size_t)n * 4), sp(d_perm, (size_t)n * 4), so(d_offsets, ((size_t)ncolours + 1) * 4);
    if (sc.meets(sp) || sc.meets(so) || sp.meets(so)) {
        set_error("%s: %s overlap", fn, sc.meets(sp) ? "d_colour and d_perm" : sc.meets(so) ? "d_colour and d_offsets" : "d_perm and d_offsets");
        return PEM_E_INVALID;
    }
    PEM_ENTER(ctx);
    // two key buffers and two payload buffers for the sort
    const size_t kbytes = ((size_t)n * 8 + 255) & ~size_t(255), vbytes = ((size_t)n * 4 + 255) & ~size_t(255);
    PEM_TRY(ctx->colour_scratch.reserve(2 * kbytes + 2 * vbytes));
    char *const base = ctx->colour_scratch.as<char>();
    uint64_t *k0 = reinterpret_cast<uint64_t *>(base), *k1 = reinterpret_cast<uint64_t *>(base + kbytes), *keys = k0;
    uint32_t *v0 = reinterpret_cast<uint32_t *>(base + 2 * kbytes), *v1 = reinterpret_cast<uint32_t *>(base + 2 * kbytes + vbytes), *verts = v0;
    PEM_TRY(zero_flags(ctx));
    if (n) {
        PEM_LAUNCH(ctx, order_keys_kernel, grid_for((size_t)n, 256), 256, d_colour, (long long)n, (int)ncolours, k0, v0, ctx->d_flags);
        PEM_TRY(radix_sort_u64_u32(ctx, k0, k1, v0, v1, (size_t)n, ncolours > 1 ? bits_for((uint64_t)ncolours) : 0, &keys, &verts));
    }
    const size_t threads = (size_t)n > (size_t)ncolours + 1 ? (size_t)n : (size_t)ncolours + 1;
    PEM_LAUNCH(ctx, order_finish_kernel, grid_for(threads, 256), 256, keys, verts, (long long)n, (int)ncolours, d_perm, d_offsets);
    int hf[NUM_FLAGS];
    PEM_TRY(read_flags(ctx, hf));   // (synchronises: the one wait of the call)
    PEM_TRY(check_internal(hf));
    if (hf[FLAG_RANGE]) {
        set_error("%s: a colour is outside [0, %d)", fn, ncolours);
        return PEM_E_INVALID;
    }
    return PEM_OK;
}
