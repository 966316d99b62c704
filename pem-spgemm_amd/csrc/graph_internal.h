// graph_internal.h -- what the graph routines share (colour.hip, components.hip, aggregate.hip): the walk over the entries of a line
// of 16 vertices, the vertex priorities and "beats", the kernel arguments and the (symmetric, hash) dispatch, the entry checks, the
// carving of pem_ctx::graph_scratch and the host's round loop.  These walks never read a value and fold with order-free LDS
// atomics only, so the visitor form costs nothing; the numeric walks (mxv.hip and its kin) stage values and keep their own loops.
#pragma once
#include "spgemm_internal.h"
#include "tiled_internal.h"
#include "mx_internal.h"
#include <climits>
#include <type_traits>

namespace pem {

// ---- the line walk ----
// what a walk reads of one orientation of a tiling: the arguments of frontier_kernel
struct LineSide {
    const int *lptr, *poff, *pbase, *pminor;
    const uint8_t *rci;
};

// the row walk reads the tiling as built, the column walk the schedule of ensure_mx_cols (null until then: walked only when !symmetric)
inline void line_sides(const pem_tiled *A, LineSide *rows, LineSide *cols)
{
    *rows = LineSide{A->tile_rowptr.as<int>(), A->tile_nnz_ptr.as<int>(), nullptr, A->tile_colidx.as<int>(), A->rowcolidx.as<uint8_t>()};
    *cols = LineSide{A->tile_colptr.as<int>(), A->mx_csc_off.as<int>(), A->mx_csc_base.as<int>(), A->tile_rowidx.as<int>(), A->mx_rci_t.as<uint8_t>()};
}

// One orientation's walk for line L, one wave, chunks of 64 entries: entry(major, j) for every stored entry, in the lane that holds
// it -- vertex 16 L + major is the near end, j the far end -- and chunk_done() after every chunk with the lanes converged
// (wave-uniform result); a true one ends the walk and is returned.
template <bool COL, class Entry, class Chunk>
__device__ __forceinline__ bool line_walk(const LineSide &S, const long long L, const int lane, Entry entry, Chunk chunk_done)
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
        if (e < e_end) {
            const unsigned rc = S.rci[COL ? t_base + (e - t_off) : e];
            entry(rc >> 4, 16 * (long long)t_minor + (rc & 15u));
        }
        if (chunk_done()) return true;
        // the next chunk starts in the tile of entry eb + 63, or in the one after it
        int pn = pc + ti_last;
        if (eb + 64 < e_end && pn + 1 < p1 && S.poff[pn + 1] <= eb + 64) ++pn;
        pc = pn;
    }
    return false;
}

// ---- priorities ----
__host__ __device__ __forceinline__ uint32_t fmix32(uint32_t h)
{
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

template <bool HASH>
__device__ __forceinline__ uint32_t vertex_priority(const long long v, const uint32_t seed_term, const uint32_t *__restrict__ prio)
{
    return HASH ? fmix32((uint32_t)v + seed_term) : prio[v];
}

// u beats v: the larger priority, ties to the lower index
__device__ __forceinline__ bool beats(const uint32_t pu, const long long u, const uint32_t pv, const long long v)
{
    return pu > pv || (pu == pv && u < v);
}

// never 0; u beats v exactly where beat_key(u) > beat_key(v)
__device__ __forceinline__ unsigned long long beat_key(const uint32_t prio, const long long v)
{
    return (((unsigned long long)prio << 31) | (unsigned long long)(INT32_MAX - (int)v)) + 1ull;
}

// ---- kernel arguments and their dispatch ----
struct GraphArgs {
    LineSide R, Cs;
    long long nlines, n;
    uint32_t seed_term;
    const uint32_t *prio;   // null: the hash
};

inline GraphArgs graph_args(const pem_tiled *A, uint32_t seed = 0, const uint32_t *d_priority = nullptr)
{
    GraphArgs g;
    line_sides(A, &g.R, &g.Cs);
    g.nlines = A->tile_rows;
    g.n = A->rows;
    g.seed_term = seed * 0x9E3779B9u;
    g.prio = d_priority;
    return g;
}

inline unsigned line_grid(const GraphArgs &g) { return grid_for((size_t)g.nlines * 64, 256); }

// f(SYM, HASH) with the flags as std::bool_constant values: decltype(sym)::value is a template argument
template <class F>
void graph_dispatch(const bool symmetric, const bool hash, F f)
{
    if (symmetric)
        hash ? f(std::true_type{}, std::true_type{}) : f(std::true_type{}, std::false_type{});
    else
        hash ? f(std::false_type{}, std::true_type{}) : f(std::false_type{}, std::false_type{});
}

// the kernel-stat name "kernel<rows|both,hash|priority tail>" (kernel and tail are literals)
#define GRAPH_KERNEL_NAME(kernel, SYM, HASH, tail)                                        \
    ((SYM) ? ((HASH) ? kernel "<rows,hash" tail ">" : kernel "<rows,priority" tail ">")   \
           : ((HASH) ? kernel "<both,hash" tail ">" : kernel "<both,priority" tail ">"))

// ---- host: entry checks, scratch, rounds ----
// The checks the entry points open with.  all_there: no required pointer is null; needs: "a colouring needs", ...; distance: MIS only.
inline pem_status graph_enter(const char *fn, const bool all_there, const pem_tiled *A, const char *needs, const int symmetric, const int distance = 1)
{
    if (!all_there) {
        set_error("%s: null argument", fn);
        return PEM_E_INVALID;
    }
    if (A->rows != A->cols) {
        set_error("%s: the tiling is %d x %d; %s a square one", fn, A->rows, A->cols, needs);
        return PEM_E_INVALID;
    }
    if (distance != 1 && distance != 2) {
        set_error("%s: distance must be 1 or 2 (got %d)", fn, distance);
        return PEM_E_INVALID;
    }
    if (!fr_flag_ok(symmetric)) {
        set_error("%s: symmetric must be 0 or 1 (got %d)", fn, symmetric);
        return PEM_E_INVALID;
    }
    return PEM_OK;
}

// One sub-buffer of the context's graph scratch: *slot gets the address of `count` T's.  Every sub-buffer starts on 256 bytes.
struct ScratchPart {
    void *slot;
    size_t bytes;
    template <class T>
    ScratchPart(T **p, const size_t count) : slot(p), bytes((count * sizeof(T) + 255) & ~size_t(255))
    {
    }
};

// grows pem_ctx::graph_scratch (grow-only; every call that uses it waits before it returns) to the parts' sum and hands them out in order
inline pem_status graph_carve(pem_ctx *ctx, std::initializer_list<ScratchPart> parts)
{
    size_t total = 0;
    for (const ScratchPart &s : parts) total += s.bytes;
    PEM_TRY(ctx->graph_scratch.reserve(total));
    char *at = ctx->graph_scratch.as<char>();
    for (const ScratchPart &s : parts) {
        memcpy(s.slot, &at, sizeof at);
        at += s.bytes;
    }
    return PEM_OK;
}

// after n rounds that still left work: quiet ends the rounds there (the caller's symmetric promise was false), otherwise text -- a
// format of (fn, the rounds, n) -- is raised
struct RoundPolicy {
    bool quiet;
    const char *text;
};

// The rounds.  round(r, more, more_next) issues round r + 1's launches, which raise *more (words[r & 1]) where work is left and clear
// *more_next; the host reads the word back (4 bytes per round).  words: two int32 on the device.
template <class Round>
pem_status graph_rounds(pem_ctx *ctx, const char *fn, const long long n, int *words, const RoundPolicy policy, Round round, int *rounds)
{
    PEM_HIP(hipMemsetAsync(words, 0, 2 * sizeof(int), ctx->stream));
    int *const h_more = reinterpret_cast<int *>(ctx->h_scalars);
    int r = 0;
    for (;;) {
        int *const more = words + (r & 1);
        round(r, more, words + ((r + 1) & 1));
        PEM_TRY(launch_status(ctx));
        PEM_HIP(hipMemcpyAsync(h_more, more, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        PEM_HIP(hipStreamSynchronize(ctx->stream));
        ++r;
        if (*h_more == 0) break;
        if (r >= n) {
            if (policy.quiet) break;
            set_error(policy.text, fn, r, n);
            return PEM_E_HIP;
        }
    }
    *rounds = r;
    return PEM_OK;
}

}  // namespace pem
