// aggregate.hip -- a maximal independent set at distance 1 or 2 of a square tiling's pattern, and the MIS(2) aggregation on top of it
// (include/pem_spgemm.h: pem_tiled_mis, pem_tiled_aggregate).
//
// The graph, the priorities and "beats" are the colouring's (colour.hip): every stored off-diagonal (i, j) is the undirected edge
// {i, j}, values are never read; the priority of v is fmix32(v + seed * 0x9E3779B9) computed in registers or the caller's
// d_priority[v]; u beats v when prio[u] > prio[v], or they are equal and u < v.  The set is the sequential greedy one in "beats"
// order.  The device runs rounds on a state byte per vertex (out, in, undecided), every round from one snapshot: an undecided vertex
// with an in vertex within `distance` turns out, otherwise one that no undecided vertex within `distance` beats turns in.
//   keys   a state and "who beats whom" in one 64-bit word: 0 for out, ((prio << 31) | (INT32_MAX - v)) + 1 for undecided (1 .. 2^63),
//          all ones for in.  The maximum over a vertex and the vertices within `distance` then decides it: all ones -> out, its own
//          key -> in, anything else -> it waits.
//   round  mis_round_kernel: the line walk of colour.hip -- one wave per line of 16 vertices, chunks of 64 entries, chunk_tile_of,
//          the (major, minor) byte -- over the row line and, unless the caller promised a symmetric pattern, over the column line of
//          the same 16 vertices.  Every entry's far-end key is folded into its near end's word of the wave's 16-word LDS area (LDS
//          64-bit atomicMax behind a plain "can it raise the word" test).  Distance 1 is one launch (<decide>): the keys come from the
//          state bytes (and the hash, or a gather of the priority, where the byte says undecided).  Distance 2 is two: <hop1> writes
//          M1[v] = the maximum key over v and its neighbours for EVERY vertex (an out or in vertex relays), <hop2> folds M1 over v and
//          its neighbours and decides.  The deciding launches skip a line without an undecided vertex (they copy its 16 bytes) and
//          only fold into the words of undecided vertices; <hop1> skips nothing: a decided line's M1 is read by undecided neighbours.
//          No kernel plain-reads, at another vertex, an array the same launch writes: a round reads one state buffer and writes the
//          other, M1 is written by <hop1> and read by <hop2>.  A wave that leaves a vertex undecided raises the round's "more" word
//          by a plain store of one value; the host reads it back (4 bytes per round).
//   finish mis_finish_kernel: the 0 / 1 bytes (an undecided vertex, which only a false symmetric = 1 promise leaves, is 0) and the
//          int32 flags exclusive_scan_i32 turns into the roots' ranks; its 64-bit total is the set's size.
//   assign aggregate_seed_kernel: aggregate[v] = rank[v] at a root, -1 elsewhere, root[rank[v]] = v.  aggregate_assign_kernel, run
//          twice (pass 1: the roots' neighbours, pass 2: the vertices two steps away): the same walk; an entry whose far end holds an
//          aggregate folds that vertex's "beats" key into the near end's word, the winner is read back out of the key's low 31 bits
//          and its aggregate taken.  Each pass reads one buffer and writes the other, so pass 2 never sees what pass 2 places.
// The scratch is the colouring's (pem_ctx::colour_scratch, grow-only; every call that uses it waits before it returns).
#include "spgemm_internal.h"
#include "tiled_internal.h"
#include "mx_internal.h"
#include <climits>

using namespace pem;

namespace {

constexpr uint8_t ST_OUT = 0, ST_IN = 1, ST_UNDECIDED = 2;
constexpr unsigned long long KEY_IN = ~0ull;
enum { MIS_DECIDE = 0, MIS_HOP1 = 1, MIS_HOP2 = 2 };

__device__ __forceinline__ uint32_t agg_fmix32(uint32_t h)
{
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

// never 0; u beats v exactly where beat_key(u) > beat_key(v)
__device__ __forceinline__ unsigned long long beat_key(const uint32_t prio, const long long v)
{
    return (((unsigned long long)prio << 31) | (unsigned long long)(INT32_MAX - (int)v)) + 1ull;
}

template <bool HASH>
__device__ __forceinline__ uint32_t prio_of(const long long v, const uint32_t seed_term, const uint32_t *__restrict__ prio)
{
    return HASH ? agg_fmix32((uint32_t)v + seed_term) : prio[v];
}

template <bool HASH>
__device__ __forceinline__ unsigned long long state_key(const uint8_t s, const long long v, const uint32_t seed_term, const uint32_t *__restrict__ prio)
{
    if (s == ST_UNDECIDED) return beat_key(prio_of<HASH>(v, seed_term, prio), v);
    return s == ST_IN ? KEY_IN : 0ull;
}

// what a walk reads of one orientation of a tiling: the arguments of frontier_kernel
struct AggSide {
    const int *lptr, *poff, *pbase, *pminor;
    const uint8_t *rci;
};

// One orientation's walk for line L: every entry whose near end is wanted (a bit of want) folds fetch(far end) into the near end's
// word of m (the wave's 16 words) by maximum.  The plain read only skips an atomic that could not raise the word (words only rise).
template <bool COL, class F>
__device__ __forceinline__ void agg_walk(const AggSide &S, const long long L, const int lane, const unsigned want, const F fetch,
                                         unsigned long long *m)
{
    const int p0 = S.lptr[L], p1 = S.lptr[L + 1];
    if (p0 >= p1) return;
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
            const unsigned major = rc >> 4;
            if (((want >> major) & 1u) != 0u) {
                const long long j = 16 * (long long)t_minor + (rc & 15u);
                const unsigned long long k = fetch(j);
                if (k > __atomic_load_n(&m[major], __ATOMIC_RELAXED)) atomicMax(&m[major], k);
            }
        }
        // the next chunk starts in the tile of entry eb + 63, or in the one after it
        int pn = pc + ti_last;
        if (eb + 64 < e_end && pn + 1 < p1 && S.poff[pn + 1] <= eb + 64) ++pn;
        pc = pn;
    }
}

// One launch of a round.  MIS_DECIDE: state_out = state_in with every undecided vertex decided from the keys within distance 1.
// MIS_HOP1: m1_out[v] = the maximum key over v and its neighbours, for every vertex.  MIS_HOP2: state_out decided from m1_in over v
// and its neighbours.  The deciding modes raise *more where a vertex stays undecided and clear *more_next, the next round's word
// (nobody else touches it in this launch).
template <bool SYM, bool HASH, int MODE>
__global__ void __launch_bounds__(256) mis_round_kernel(const AggSide R, const AggSide Cs, const long long nlines, const long long n,
                                                        const uint32_t seed_term, const uint32_t *__restrict__ prio,
                                                        const uint8_t *__restrict__ state_in, const unsigned long long *__restrict__ m1_in,
                                                        uint8_t *__restrict__ state_out, unsigned long long *__restrict__ m1_out, int *more,
                                                        int *more_next)
{
    __shared__ unsigned long long s_m[4 * 16];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long L = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (MODE != MIS_HOP1 && blockIdx.x == 0 && threadIdx.x == 0) *more_next = 0;
    if (L >= nlines) return;   // (wave-uniform)
    const long long v = 16 * L + lane;
    const bool mine = lane < 16 && v < n;
    uint8_t s = mine ? state_in[v] : ST_OUT;
    unsigned want = 0xFFFFu;
    if constexpr (MODE != MIS_HOP1) {
        want = (unsigned)__ballot(mine && s == ST_UNDECIDED);
        if (want == 0u) {   // (wave-uniform) nothing left to decide in this line
            if (mine) state_out[v] = s;
            return;
        }
    }
    const unsigned long long own = mine ? state_key<HASH>(s, v, seed_term, prio) : 0ull;
    unsigned long long *const m = s_m + wv * 16;
    if (lane < 16) m[lane] = (MODE == MIS_HOP2 && mine) ? m1_in[v] : own;
    mx_wave_sync();
    auto fetch = [&](const long long j) -> unsigned long long {
        if constexpr (MODE == MIS_HOP2)
            return m1_in[j];
        else
            return state_key<HASH>(state_in[j], j, seed_term, prio);
    };
    agg_walk<false>(R, L, lane, want, fetch, m);
    if constexpr (!SYM) agg_walk<true>(Cs, L, lane, want, fetch, m);
    mx_wave_sync();
    if constexpr (MODE == MIS_HOP1) {
        if (mine) m1_out[v] = m[lane];
    } else {
        if (mine) {
            if (s == ST_UNDECIDED) {
                const unsigned long long top = m[lane];
                if (top == KEY_IN)
                    s = ST_OUT;
                else if (top == own)
                    s = ST_IN;
            }
            state_out[v] = s;
        }
        if (__ballot(mine && s == ST_UNDECIDED) != 0ull && lane == 0) *more = 1;
    }
}

// in_set = the 0 / 1 bytes of the final states (in_set may be state: element-wise), flag = the same as int32 for the scan
__global__ void __launch_bounds__(256) mis_finish_kernel(const uint8_t *state, uint8_t *in_set, int *__restrict__ flag, const long long n)
{
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const uint8_t in = state[v] == ST_IN ? 1 : 0;
    in_set[v] = in;
    flag[v] = in;
}

// aggregate[v] = the root's number at a root, -1 elsewhere; root[number] = the root (root, when given, was filled with -1)
__global__ void __launch_bounds__(256) aggregate_seed_kernel(const uint8_t *__restrict__ in_set, const int *__restrict__ rank, const long long n,
                                                             int *__restrict__ agg, int *__restrict__ root)
{
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const bool in = in_set[v] != 0;
    const int id = rank[v];
    agg[v] = in ? id : -1;
    if (in && root) root[id] = (int)v;
}

// one assignment pass: agg_out = agg_in with every vertex without an aggregate taking the aggregate of the placed neighbour that
// beats the other placed neighbours (-1 where it has none)
template <bool SYM, bool HASH>
__global__ void __launch_bounds__(256) aggregate_assign_kernel(const AggSide R, const AggSide Cs, const long long nlines, const long long n,
                                                               const uint32_t seed_term, const uint32_t *__restrict__ prio,
                                                               const int *__restrict__ agg_in, int *__restrict__ agg_out)
{
    __shared__ unsigned long long s_m[4 * 16];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long L = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (L >= nlines) return;   // (wave-uniform)
    const long long v = 16 * L + lane;
    const bool mine = lane < 16 && v < n;
    int a = mine ? agg_in[v] : 0;
    const unsigned want = (unsigned)__ballot(mine && a < 0);
    if (want == 0u) {   // (wave-uniform) every vertex of the line is placed
        if (mine) agg_out[v] = a;
        return;
    }
    unsigned long long *const m = s_m + wv * 16;
    if (lane < 16) m[lane] = 0ull;
    mx_wave_sync();
    auto fetch = [&](const long long j) -> unsigned long long {
        return agg_in[j] >= 0 ? beat_key(prio_of<HASH>(j, seed_term, prio), j) : 0ull;
    };
    agg_walk<false>(R, L, lane, want, fetch, m);
    if constexpr (!SYM) agg_walk<true>(Cs, L, lane, want, fetch, m);
    mx_wave_sync();
    if (mine) {
        if (a < 0) {
            const unsigned long long top = m[lane];
            if (top != 0ull) a = agg_in[INT32_MAX - (int)((top - 1ull) & 0x7FFFFFFFull)];   // the winner's vertex number is in the key
        }
        agg_out[v] = a;
    }
}

struct MisArgs {
    AggSide R, Cs;
    long long nlines, n;
    uint32_t seed_term;
    const uint32_t *prio;
};

template <bool SYM, bool HASH, int MODE>
void mis_launch_one(pem_ctx *ctx, const char *name, const MisArgs &a, const uint8_t *sin, const unsigned long long *m1_in, uint8_t *sout,
                    unsigned long long *m1_out, int *more, int *more_next)
{
    PEM_LAUNCH_NAMED(ctx, name, (mis_round_kernel<SYM, HASH, MODE>), grid_for((size_t)a.nlines * 64, 256), 256, a.R, a.Cs, a.nlines, a.n,
                     a.seed_term, a.prio, sin, m1_in, sout, m1_out, more, more_next);
}

// one round: sout = the states after a round on sin
template <bool SYM, bool HASH>
void mis_round(pem_ctx *ctx, int distance, const MisArgs &a, const uint8_t *sin, uint8_t *sout, unsigned long long *m1, int *more, int *more_next)
{
#define MIS_NAME(mode) (SYM ? (HASH ? "mis_round_kernel<rows,hash," mode ">" : "mis_round_kernel<rows,priority," mode ">") \
                            : (HASH ? "mis_round_kernel<both,hash," mode ">" : "mis_round_kernel<both,priority," mode ">"))
    if (distance == 1) {
        mis_launch_one<SYM, HASH, MIS_DECIDE>(ctx, MIS_NAME("decide"), a, sin, nullptr, sout, nullptr, more, more_next);
    } else {
        mis_launch_one<SYM, HASH, MIS_HOP1>(ctx, MIS_NAME("hop1"), a, sin, nullptr, nullptr, m1, nullptr, nullptr);
        mis_launch_one<SYM, HASH, MIS_HOP2>(ctx, MIS_NAME("hop2"), a, sin, m1, sout, nullptr, more, more_next);
    }
#undef MIS_NAME
}

// The rounds: buf[0] starts undecided, round r + 1 reads buf[r & 1] and writes the other.  *at: the buffer that holds the final
// states.  words: the two "more" words.
pem_status mis_rounds(pem_ctx *ctx, const char *fn, int distance, int symmetric, const MisArgs &a, uint8_t *const buf[2], unsigned long long *m1,
                      int *words, int *rounds, int *at)
{
    PEM_HIP(hipMemsetAsync(buf[0], ST_UNDECIDED, (size_t)a.n, ctx->stream));
    PEM_HIP(hipMemsetAsync(words, 0, 2 * sizeof(int), ctx->stream));
    int *const h_more = reinterpret_cast<int *>(ctx->h_scalars);
    const bool hash = a.prio == nullptr;
    int r = 0;
    for (;;) {   // round r + 1 raises words[r & 1] and clears the other word
        int *const more = words + (r & 1), *const more_next = words + ((r + 1) & 1);
        const uint8_t *sin = buf[r & 1];
        uint8_t *sout = buf[(r + 1) & 1];
        if (symmetric) {
            if (hash) mis_round<true, true>(ctx, distance, a, sin, sout, m1, more, more_next);
            else mis_round<true, false>(ctx, distance, a, sin, sout, m1, more, more_next);
        } else {
            if (hash) mis_round<false, true>(ctx, distance, a, sin, sout, m1, more, more_next);
            else mis_round<false, false>(ctx, distance, a, sin, sout, m1, more, more_next);
        }
        PEM_TRY(launch_status(ctx));
        PEM_HIP(hipMemcpyAsync(h_more, more, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        PEM_HIP(hipStreamSynchronize(ctx->stream));
        ++r;
        if (*h_more == 0) break;
        if (r >= a.n) {   // (every round decides the best undecided vertex at least)
            if (symmetric) break;   // the promise was false
            set_error("%s: internal: vertices left undecided after %d rounds", fn, r);
            return PEM_E_HIP;
        }
    }
    *rounds = r;
    *at = r & 1;
    return PEM_OK;
}

MisArgs mis_args(const pem_tiled *A, uint32_t seed, const uint32_t *d_priority)
{
    MisArgs a;
    a.R = AggSide{A->tile_rowptr.as<int>(), A->tile_nnz_ptr.as<int>(), nullptr, A->tile_colidx.as<int>(), A->rowcolidx.as<uint8_t>()};
    a.Cs = AggSide{A->tile_colptr.as<int>(), A->mx_csc_off.as<int>(), A->mx_csc_base.as<int>(), A->tile_rowidx.as<int>(), A->mx_rci_t.as<uint8_t>()};
    a.nlines = A->tile_rows;
    a.n = A->rows;
    a.seed_term = seed * 0x9E3779B9u;
    a.prio = d_priority;
    return a;
}

inline size_t pad256(size_t bytes) { return (bytes + 255) & ~size_t(255); }

template <bool SYM>
void assign_launch(pem_ctx *ctx, const MisArgs &a, const int *agg_in, int *agg_out)
{
    const unsigned grid = grid_for((size_t)a.nlines * 64, 256);
    if (a.prio == nullptr)
        PEM_LAUNCH_NAMED(ctx, SYM ? "aggregate_assign_kernel<rows,hash>" : "aggregate_assign_kernel<both,hash>", (aggregate_assign_kernel<SYM, true>),
                         grid, 256, a.R, a.Cs, a.nlines, a.n, a.seed_term, a.prio, agg_in, agg_out);
    else
        PEM_LAUNCH_NAMED(ctx, SYM ? "aggregate_assign_kernel<rows,priority>" : "aggregate_assign_kernel<both,priority>",
                         (aggregate_assign_kernel<SYM, false>), grid, 256, a.R, a.Cs, a.nlines, a.n, a.seed_term, a.prio, agg_in, agg_out);
}

}  // namespace

extern "C" pem_status pem_tiled_mis(pem_ctx *ctx, const pem_tiled *A, int distance, int symmetric, uint32_t seed, const uint32_t *d_priority,
                                    uint8_t *d_in_set, int64_t *count, int32_t *rounds)
{
    const char *fn = "pem_tiled_mis";
    if (!ctx || !A || !d_in_set || !count || !rounds) {
        set_error("%s: null argument", fn);
        return PEM_E_INVALID;
    }
    if (A->rows != A->cols) {
        set_error("%s: the tiling is %d x %d; an independent set needs a square one", fn, A->rows, A->cols);
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
    const long long n = A->rows;
    if (Span(d_priority, (size_t)n * 4).meets(Span(d_in_set, (size_t)n))) {
        set_error("%s: d_priority and d_in_set overlap", fn);
        return PEM_E_INVALID;
    }
    *count = 0;
    *rounds = 0;
    if (n == 0) return PEM_OK;
    PEM_ENTER(ctx);
    if (!symmetric) PEM_TRY(ensure_mx_cols(ctx, A));
    // the second state buffer, M1, the flags (the scan writes its total behind the ranks), the two round words
    const size_t sbytes = pad256((size_t)n), mbytes = pad256((size_t)n * 8), rbytes = pad256(((size_t)n + 1) * sizeof(int));
    PEM_TRY(ctx->colour_scratch.reserve(sbytes + mbytes + rbytes + 256));
    char *const base = ctx->colour_scratch.as<char>();
    uint8_t *const buf[2] = {d_in_set, reinterpret_cast<uint8_t *>(base)};
    unsigned long long *const m1 = reinterpret_cast<unsigned long long *>(base + sbytes);
    int *const rank = reinterpret_cast<int *>(base + sbytes + mbytes);
    int *const words = reinterpret_cast<int *>(base + sbytes + mbytes + rbytes);
    const MisArgs a = mis_args(A, seed, d_priority);
    int r = 0, at = 0;
    PEM_TRY(zero_flags(ctx));
    PEM_TRY(mis_rounds(ctx, fn, distance, symmetric, a, buf, m1, words, &r, &at));
    PEM_LAUNCH(ctx, mis_finish_kernel, grid_for((size_t)n, 256), 256, buf[at], d_in_set, rank, n);
    PEM_TRY(exclusive_scan_i32(ctx, rank, rank, (size_t)n, ctx->d_scalars));
    PEM_TRY(launch_status(ctx));
    int64_t total = 0;
    PEM_TRY(read_scalars(ctx, ctx->d_scalars, 1, &total));
    *count = total;
    *rounds = r;
    return PEM_OK;
}

extern "C" pem_status pem_tiled_aggregate(pem_ctx *ctx, const pem_tiled *A, int symmetric, uint32_t seed, const uint32_t *d_priority,
                                          int32_t *d_aggregate, int32_t *d_root, int64_t *naggregates, int32_t *rounds)
{
    const char *fn = "pem_tiled_aggregate";
    if (!ctx || !A || !d_aggregate || !naggregates || !rounds) {
        set_error("%s: null argument", fn);
        return PEM_E_INVALID;
    }
    if (A->rows != A->cols) {
        set_error("%s: the tiling is %d x %d; an aggregation needs a square one", fn, A->rows, A->cols);
        return PEM_E_INVALID;
    }
    if (!fr_flag_ok(symmetric)) {
        set_error("%s: symmetric must be 0 or 1 (got %d)", fn, symmetric);
        return PEM_E_INVALID;
    }
    const long long n = A->rows;
    const Span sp(d_priority, (size_t)n * 4), sa(d_aggregate, (size_t)n * 4), sr(d_root, (size_t)n * 4);
    if (sp.meets(sa) || sp.meets(sr) || sa.meets(sr)) {
        set_error("%s: %s overlap", fn, sp.meets(sa) ? "d_priority and d_aggregate" : sp.meets(sr) ? "d_priority and d_root" : "d_aggregate and d_root");
        return PEM_E_INVALID;
    }
    *naggregates = 0;
    *rounds = 0;
    if (n == 0) return PEM_OK;
    PEM_ENTER(ctx);
    if (!symmetric) PEM_TRY(ensure_mx_cols(ctx, A));
    // two state buffers, M1, the flags and ranks, the second aggregate buffer, the two round words
    const size_t sbytes = pad256((size_t)n), mbytes = pad256((size_t)n * 8), rbytes = pad256(((size_t)n + 1) * sizeof(int));
    PEM_TRY(ctx->colour_scratch.reserve(2 * sbytes + mbytes + 2 * rbytes + 256));
    char *const base = ctx->colour_scratch.as<char>();
    uint8_t *const buf[2] = {reinterpret_cast<uint8_t *>(base), reinterpret_cast<uint8_t *>(base + sbytes)};
    unsigned long long *const m1 = reinterpret_cast<unsigned long long *>(base + 2 * sbytes);
    int *const rank = reinterpret_cast<int *>(base + 2 * sbytes + mbytes);
    int *const agg1 = reinterpret_cast<int *>(base + 2 * sbytes + mbytes + rbytes);
    int *const words = reinterpret_cast<int *>(base + 2 * sbytes + mbytes + 2 * rbytes);
    const MisArgs a = mis_args(A, seed, d_priority);
    const unsigned egrid = grid_for((size_t)n, 256);
    int r = 0, at = 0;
    PEM_TRY(zero_flags(ctx));
    PEM_TRY(mis_rounds(ctx, fn, 2, symmetric, a, buf, m1, words, &r, &at));
    PEM_LAUNCH(ctx, mis_finish_kernel, egrid, 256, buf[at], buf[at], rank, n);
    PEM_TRY(exclusive_scan_i32(ctx, rank, rank, (size_t)n, ctx->d_scalars));
    if (d_root) PEM_HIP(hipMemsetAsync(d_root, 0xFF, (size_t)n * sizeof(int), ctx->stream));
    PEM_LAUNCH(ctx, aggregate_seed_kernel, egrid, 256, buf[at], rank, n, d_aggregate, d_root);
    if (symmetric) {
        assign_launch<true>(ctx, a, d_aggregate, agg1);
        assign_launch<true>(ctx, a, agg1, d_aggregate);
    } else {
        assign_launch<false>(ctx, a, d_aggregate, agg1);
        assign_launch<false>(ctx, a, agg1, d_aggregate);
    }
    PEM_TRY(launch_status(ctx));
    int64_t total = 0;
    PEM_TRY(read_scalars(ctx, ctx->d_scalars, 1, &total));
    *naggregates = total;
    *rounds = r;
    return PEM_OK;
}
