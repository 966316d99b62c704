// aggregate.hip -- a maximal independent set at distance 1 or 2 of a square tiling's pattern, and the MIS(2) aggregation on top of it
// (include/pem_spgemm.h: pem_tiled_mis, pem_tiled_aggregate).
//
// The graph, the priorities and "beats" are the colouring's (colour.hip, graph_internal.h): every stored off-diagonal (i, j) is the undirected edge
// {i, j}, values are never read; the priority of v is fmix32(v + seed * 0x9E3779B9) computed in registers or the caller's
// d_priority[v]; u beats v when prio[u] > prio[v], or they are equal and u < v.  The set is the sequential greedy one in "beats"
// order.  The device runs rounds on a state byte per vertex (out, in, undecided), every round from one snapshot: an undecided vertex
// with an in vertex within `distance` turns out, otherwise one that no undecided vertex within `distance` beats turns in.
//   keys   a state and "who beats whom" in one 64-bit word: 0 for out, ((prio << 31) | (INT32_MAX - v)) + 1 for undecided (1 .. 2^63),
//          all ones for in.  The maximum over a vertex and the vertices within `distance` then decides it: all ones -> out, its own
//          key -> in, anything else -> it waits.
//   round  mis_round_kernel: the line walk of graph_internal.h (line_walk) -- one wave per line of 16 vertices, chunks of 64
//          entries -- over the row line and, unless the caller promised a symmetric pattern, over the column line of
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
// The scratch is the graph routines' (pem_ctx::graph_scratch, carved by graph_carve); the host's round loop is graph_rounds.
#include "spgemm_internal.h"
#include "tiled_internal.h"
#include "graph_internal.h"

using namespace pem;

namespace {

constexpr uint8_t ST_OUT = 0, ST_IN = 1, ST_UNDECIDED = 2;
constexpr unsigned long long KEY_IN = ~0ull;
enum { MIS_DECIDE = 0, MIS_HOP1 = 1, MIS_HOP2 = 2 };

template <bool HASH>
__device__ __forceinline__ unsigned long long state_key(const uint8_t s, const long long v, const uint32_t seed_term, const uint32_t *__restrict__ prio)
{
    if (s == ST_UNDECIDED) return beat_key(vertex_priority<HASH>(v, seed_term, prio), v);
    return s == ST_IN ? KEY_IN : 0ull;
}

// What a walk of line L does with an entry: where its near end is wanted (a bit of want) it folds fetch(far end) into the near end's
// word of m (the wave's 16 words) by maximum.  The plain read only skips an atomic that could not raise the word (words only rise).
template <bool SYM, class F>
__device__ __forceinline__ void max_walks(const GraphArgs &g, const long long L, const int lane, const unsigned want, const F fetch,
                                          unsigned long long *m)
{
    auto entry = [&](const unsigned major, const long long j) {
        if (((want >> major) & 1u) != 0u) {
            const unsigned long long k = fetch(j);
            if (k > __atomic_load_n(&m[major], __ATOMIC_RELAXED)) atomicMax(&m[major], k);
        }
    };
    auto walk_on = [] { return false; };
    line_walk<false>(g.R, L, lane, entry, walk_on);
    if constexpr (!SYM) line_walk<true>(g.Cs, L, lane, entry, walk_on);
}

// One launch of a round.  MIS_DECIDE: state_out = state_in with every undecided vertex decided from the keys within distance 1.
// MIS_HOP1: m1_out[v] = the maximum key over v and its neighbours, for every vertex.  MIS_HOP2: state_out decided from m1_in over v
// and its neighbours.  The deciding modes raise *more where a vertex stays undecided and clear *more_next, the next round's word
// (nobody else touches it in this launch).
template <bool SYM, bool HASH, int MODE>
__global__ void __launch_bounds__(256) mis_round_kernel(const GraphArgs g, const uint8_t *__restrict__ state_in,
                                                        const unsigned long long *__restrict__ m1_in, uint8_t *__restrict__ state_out,
                                                        unsigned long long *__restrict__ m1_out, int *more, int *more_next)
{
    __shared__ unsigned long long s_m[4 * 16];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long L = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (MODE != MIS_HOP1 && blockIdx.x == 0 && threadIdx.x == 0) *more_next = 0;
    if (L >= g.nlines) return;   // (wave-uniform)
    const long long v = 16 * L + lane;
    const bool mine = lane < 16 && v < g.n;
    uint8_t s = mine ? state_in[v] : ST_OUT;
    unsigned want = 0xFFFFu;
    if constexpr (MODE != MIS_HOP1) {
        want = (unsigned)__ballot(mine && s == ST_UNDECIDED);
        if (want == 0u) {   // (wave-uniform) nothing left to decide in this line
            if (mine) state_out[v] = s;
            return;
        }
    }
    const unsigned long long own = mine ? state_key<HASH>(s, v, g.seed_term, g.prio) : 0ull;
    unsigned long long *const m = s_m + wv * 16;
    if (lane < 16) m[lane] = (MODE == MIS_HOP2 && mine) ? m1_in[v] : own;
    mx_wave_sync();
    auto fetch = [&](const long long j) -> unsigned long long {
        if constexpr (MODE == MIS_HOP2)
            return m1_in[j];
        else
            return state_key<HASH>(state_in[j], j, g.seed_term, g.prio);
    };
    max_walks<SYM>(g, L, lane, want, fetch, m);
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
__global__ void __launch_bounds__(256) aggregate_assign_kernel(const GraphArgs g, const int *__restrict__ agg_in, int *__restrict__ agg_out)
{
    __shared__ unsigned long long s_m[4 * 16];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long L = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (L >= g.nlines) return;   // (wave-uniform)
    const long long v = 16 * L + lane;
    const bool mine = lane < 16 && v < g.n;
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
        return agg_in[j] >= 0 ? beat_key(vertex_priority<HASH>(j, g.seed_term, g.prio), j) : 0ull;
    };
    max_walks<SYM>(g, L, lane, want, fetch, m);
    mx_wave_sync();
    if (mine) {
        if (a < 0) {
            const unsigned long long top = m[lane];
            if (top != 0ull) a = agg_in[INT32_MAX - (int)((top - 1ull) & 0x7FFFFFFFull)];   // the winner's vertex number is in the key
        }
        agg_out[v] = a;
    }
}

// The rounds: buf[0] starts undecided, round r + 1 reads buf[r & 1] and writes the other -- one launch at distance 1, hop1 into m1
// then hop2 at distance 2.  Every round decides the best undecided vertex at least, so only a false promise takes more than n.
pem_status mis_rounds(pem_ctx *ctx, const char *fn, int distance, int symmetric, const GraphArgs &g, uint8_t *const buf[2], unsigned long long *m1,
                      int *words, int *rounds)
{
    PEM_HIP(hipMemsetAsync(buf[0], ST_UNDECIDED, (size_t)g.n, ctx->stream));
    return graph_rounds(
        ctx, fn, g.n, words, RoundPolicy{symmetric != 0, "%s: internal: vertices left undecided after %d rounds"},
        [&](const int r, int *more, int *more_next) {
            const uint8_t *const sin = buf[r & 1];
            uint8_t *const sout = buf[(r + 1) & 1];
            graph_dispatch(symmetric, g.prio == nullptr, [&](auto sym, auto hash) {
                constexpr bool SYM = decltype(sym)::value, HASH = decltype(hash)::value;
                if (distance == 1) {
                    PEM_LAUNCH_NAMED(ctx, GRAPH_KERNEL_NAME("mis_round_kernel", SYM, HASH, ",decide"), (mis_round_kernel<SYM, HASH, MIS_DECIDE>),
                                     line_grid(g), 256, g, sin, nullptr, sout, nullptr, more, more_next);
                } else {
                    PEM_LAUNCH_NAMED(ctx, GRAPH_KERNEL_NAME("mis_round_kernel", SYM, HASH, ",hop1"), (mis_round_kernel<SYM, HASH, MIS_HOP1>),
                                     line_grid(g), 256, g, sin, nullptr, nullptr, m1, nullptr, nullptr);
                    PEM_LAUNCH_NAMED(ctx, GRAPH_KERNEL_NAME("mis_round_kernel", SYM, HASH, ",hop2"), (mis_round_kernel<SYM, HASH, MIS_HOP2>),
                                     line_grid(g), 256, g, sin, m1, sout, nullptr, more, more_next);
                }
            });
        },
        rounds);
}

void assign_launch(pem_ctx *ctx, int symmetric, const GraphArgs &g, const int *agg_in, int *agg_out)
{
    graph_dispatch(symmetric, g.prio == nullptr, [&](auto sym, auto hash) {
        constexpr bool SYM = decltype(sym)::value, HASH = decltype(hash)::value;
        PEM_LAUNCH_NAMED(ctx, GRAPH_KERNEL_NAME("aggregate_assign_kernel", SYM, HASH, ""), (aggregate_assign_kernel<SYM, HASH>), line_grid(g), 256, g,
                         agg_in, agg_out);
    });
}

}  // namespace

extern "C" pem_status pem_tiled_mis(pem_ctx *ctx, const pem_tiled *A, int distance, int symmetric, uint32_t seed, const uint32_t *d_priority,
                                    uint8_t *d_in_set, int64_t *count, int32_t *rounds)
{
    const char *fn = "pem_tiled_mis";
    PEM_TRY(graph_enter(fn, ctx && A && d_in_set && count && rounds, A, "an independent set needs", symmetric, distance));
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
    uint8_t *buf[2] = {d_in_set, nullptr};
    unsigned long long *m1;
    int *rank, *words;
    PEM_TRY(graph_carve(ctx, {{&buf[1], (size_t)n}, {&m1, (size_t)n}, {&rank, (size_t)n + 1}, {&words, 2}}));
    const GraphArgs g = graph_args(A, seed, d_priority);
    int r = 0;
    PEM_TRY(zero_flags(ctx));
    PEM_TRY(mis_rounds(ctx, fn, distance, symmetric, g, buf, m1, words, &r));
    const int at = r & 1;   // the buffer that holds the final states
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
    PEM_TRY(graph_enter(fn, ctx && A && d_aggregate && naggregates && rounds, A, "an aggregation needs", symmetric));
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
    uint8_t *buf[2];
    unsigned long long *m1;
    int *rank, *agg1, *words;
    PEM_TRY(graph_carve(ctx, {{&buf[0], (size_t)n}, {&buf[1], (size_t)n}, {&m1, (size_t)n}, {&rank, (size_t)n + 1}, {&agg1, (size_t)n + 1}, {&words, 2}}));
    const GraphArgs g = graph_args(A, seed, d_priority);
    const unsigned egrid = grid_for((size_t)n, 256);
    int r = 0;
    PEM_TRY(zero_flags(ctx));
    PEM_TRY(mis_rounds(ctx, fn, 2, symmetric, g, buf, m1, words, &r));
    const int at = r & 1;   // the buffer that holds the final states
    PEM_LAUNCH(ctx, mis_finish_kernel, egrid, 256, buf[at], buf[at], rank, n);
    PEM_TRY(exclusive_scan_i32(ctx, rank, rank, (size_t)n, ctx->d_scalars));
    if (d_root) PEM_HIP(hipMemsetAsync(d_root, 0xFF, (size_t)n * sizeof(int), ctx->stream));
    PEM_LAUNCH(ctx, aggregate_seed_kernel, egrid, 256, buf[at], rank, n, d_aggregate, d_root);
    assign_launch(ctx, symmetric, g, d_aggregate, agg1);
    assign_launch(ctx, symmetric, g, agg1, d_aggregate);
    PEM_TRY(launch_status(ctx));
    int64_t total = 0;
    PEM_TRY(read_scalars(ctx, ctx->d_scalars, 1, &total));
    *naggregates = total;
    *rounds = r;
    return PEM_OK;
}
