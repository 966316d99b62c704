// colour.hip -- greedy graph colouring of a square tiling's pattern and the permutation that sorts the vertices by colour
// (include/pem_spgemm.h: pem_tiled_colour, pem_colour_order).
//
// The graph: every stored off-diagonal (i, j) is the undirected edge {i, j}; values are never read.  Every vertex has a priority --
// fmix32(v + seed * 0x9E3779B9) computed in registers, or the caller's d_priority[v] -- larger first, ties to the lower index, and
// colour[v] is the smallest colour no neighbour of higher priority holds: the sequential greedy colouring in that order.  The rounds
// are Jones-Plassmann's, which reproduce it exactly: in a round every uncoloured vertex none of whose uncoloured neighbours beats it
// takes the smallest colour its coloured neighbours leave free.
//   round  colour_round_kernel: the line walk of graph_internal.h (line_walk) -- one wave per line of 16 vertices, chunks of 64
//          entries -- over the row line and, unless the caller promised a symmetric pattern, over the column line of the same 16
//          vertices (the column schedule of mxv.hip).  An entry whose far end is uncoloured and beats the
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
// The scratch of both calls is the context's (pem_ctx::graph_scratch, grow-only, carved by graph_carve); the host's round loop is
// graph_rounds.
#include "spgemm_internal.h"
#include "tiled_internal.h"
#include "graph_internal.h"

using namespace pem;

namespace {

// What a walk of line L (either orientation) does.  want: the vertices (bits) of the line whose neighbours matter; first: the pass that
// also tests the priorities (later windows only collect colours: their vertices are known to be unblocked).  my_prio: lane m < 16
// holds the priority of vertex 16 L + m, so the near end's priority is a shuffle, which needs the lanes converged: entry only
// gathers the far end's colour, and chunk_done acts on it.  chunk_done returns true when every wanted vertex is blocked (first pass
// only): nothing more can change.
template <bool SYM, bool HASH>
__device__ __forceinline__ bool colour_walks(const GraphArgs &g, const long long L, const int lane, const unsigned want, const bool first,
                                             const uint32_t my_prio, const int *__restrict__ colour_in, const int base, unsigned long long *used,
                                             unsigned *blk)
{
    unsigned major = 0;
    long long rival = -1;   // the lane's entry whose far end is uncoloured (first pass only)
    auto entry = [&](const unsigned e_major, const long long j) {
        major = e_major;
        if (((want >> e_major) & 1u) != 0u && j != 16 * L + e_major) {
            const int cj = colour_in[j];
            if (cj < 0) {
                if (first) rival = j;
            } else if (cj >= base && cj - base < 64) {
                atomicOr(&used[e_major], 1ull << (cj - base));
            }
        }
    };
    auto chunk_done = [&]() -> bool {
        if (first) {
            const uint32_t pi = (uint32_t)__shfl((int)my_prio, (int)major, 64);
            if (rival >= 0 && beats(vertex_priority<HASH>(rival, g.seed_term, g.prio), rival, pi, 16 * L + major)) atomicOr(blk, 1u << major);
            rival = -1;
            mx_wave_sync();
            if ((__builtin_amdgcn_readfirstlane(*blk) & want) == want) return true;   // (wave-uniform)
        }
        return false;
    };
    bool all_blocked = line_walk<false>(g.R, L, lane, entry, chunk_done);
    if constexpr (!SYM)
        if (!all_blocked) all_blocked = line_walk<true>(g.Cs, L, lane, entry, chunk_done);
    return all_blocked;
}

// one round: colour_out = colour_in with every unblocked uncoloured vertex coloured.  *more is raised where a vertex stays
// uncoloured; *more_next, the next round's word, is cleared (nobody else touches it in this launch).
template <bool SYM, bool HASH>
__global__ void __launch_bounds__(256) colour_round_kernel(const GraphArgs g, const int *__restrict__ colour_in, int *__restrict__ colour_out, int *more,
                                                           int *more_next)
{
    __shared__ unsigned long long s_used[4 * 16];
    __shared__ unsigned s_blk[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long L = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (blockIdx.x == 0 && threadIdx.x == 0) *more_next = 0;
    if (L >= g.nlines) return;   // (wave-uniform)
    const long long v = 16 * L + lane;
    const bool mine = lane < 16 && v < g.n;
    int c = mine ? colour_in[v] : 0;
    unsigned want = (unsigned)__ballot(mine && c < 0);
    if (want == 0u) {   // (wave-uniform) nothing left to colour in this line
        if (mine) colour_out[v] = c;
        return;
    }
    unsigned long long *const used = s_used + wv * 16;
    unsigned *const blk = s_blk + wv;
    uint32_t my_prio = 0;
    if (mine) my_prio = vertex_priority<HASH>(v, g.seed_term, g.prio);
    if (lane < 16) used[lane] = 0ull;
    if (lane == 0) *blk = 0u;
    mx_wave_sync();
    bool first = true;
    for (int base = 0; want != 0u; base += 64) {   // (wave-uniform) one trip per window of 64 colours
        if (colour_walks<SYM, HASH>(g, L, lane, want, first, my_prio, colour_in, base, used, blk)) break;
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

}  // namespace

extern "C" pem_status pem_tiled_colour(pem_ctx *ctx, const pem_tiled *A, int symmetric, uint32_t seed, const uint32_t *d_priority,
                                       int32_t *d_colour, int32_t *ncolours, int32_t *rounds)
{
    const char *fn = "pem_tiled_colour";
    PEM_TRY(graph_enter(fn, ctx && A && d_colour && ncolours && rounds, A, "a colouring needs", symmetric));
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
    int *buf[2] = {d_colour, nullptr}, *words;   // words: more[2], then the largest colour
    PEM_TRY(graph_carve(ctx, {{&buf[1], (size_t)n}, {&words, 3}}));
    const GraphArgs g = graph_args(A, seed, d_priority);
    PEM_HIP(hipMemsetAsync(buf[0], 0xFF, (size_t)n * sizeof(int), ctx->stream));   // every vertex uncoloured (-1)
    PEM_HIP(hipMemsetAsync(words + 2, 0xFF, sizeof(int), ctx->stream));
    int r = 0;
    // round r + 1 reads buf[r & 1] and writes the other; every round colours the best uncoloured vertex at least
    PEM_TRY(graph_rounds(
        ctx, fn, n, words, RoundPolicy{false, "%s: internal: vertices left uncoloured after %d rounds"},
        [&](const int at, int *more, int *more_next) {
            graph_dispatch(symmetric, d_priority == nullptr, [&](auto sym, auto hash) {
                constexpr bool SYM = decltype(sym)::value, HASH = decltype(hash)::value;
                PEM_LAUNCH_NAMED(ctx, GRAPH_KERNEL_NAME("colour_round_kernel", SYM, HASH, ""), (colour_round_kernel<SYM, HASH>), line_grid(g), 256, g,
                                 buf[at & 1], buf[(at + 1) & 1], more, more_next);
            });
        },
        &r));
    if (r & 1) PEM_HIP(hipMemcpyAsync(d_colour, buf[1], (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, ctx->stream));
    PEM_LAUNCH(ctx, colour_max_kernel, grid_for((size_t)n, 1024), 256, d_colour, n, words + 2);
    PEM_TRY(launch_status(ctx));
    int *const h_max = reinterpret_cast<int *>(ctx->h_scalars);
    PEM_HIP(hipMemcpyAsync(h_max, words + 2, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    PEM_HIP(hipStreamSynchronize(ctx->stream));
    *ncolours = *h_max + 1;
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
    uint64_t *k0, *k1, *keys;
    uint32_t *v0, *v1, *verts;
    PEM_TRY(graph_carve(ctx, {{&k0, (size_t)n}, {&k1, (size_t)n}, {&v0, (size_t)n}, {&v1, (size_t)n}}));
    keys = k0;
    verts = v0;
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
