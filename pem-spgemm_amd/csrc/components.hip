// components.hip -- the connected components of a square tiling's pattern: the smallest vertex of every vertex's component, the dense
// component ids and their count (include/pem_spgemm.h: pem_tiled_components).
//
// The graph: every stored (i, j) is the undirected edge {i, j}; values are never read.  The state is a parent array f, started at
// f[v] = v, with f[v] <= v throughout.  A round (FastSV's shortcutting, aggressive hooking and hooking onto the parent, all taken on
// one snapshot):  gp[v] = f[f[v]];  m[v] = the minimum of gp[u] over v's neighbours u;  f'[x] = min(gp[x], m[x], min{m[v] : f[v] == x}).
// f' is a minimum over a fixed set, so no order shows and the number of rounds is determined; the call ends after the first round
// with f' == f.
//   gp     components_gp_kernel: element-wise, gp[v] = f[f[v]] into the gp buffer and into fnext, the buffer the hooks min into;
//          raises the round's "changed" word where gp[v] < f[v] and clears the next round's word.
//   hook   components_hook_kernel: the line walk of graph_internal.h (line_walk) -- one wave per line of 16 vertices, chunks of 64
//          entries -- over the row line and, unless the caller promised a symmetric pattern, over the column line of the same 16
//          vertices (the column schedule of mxv.hip).  Every entry gathers gp[j] and mins it into its near
//          vertex's word of the wave's 16-word LDS area (LDS atomicMin).  After the walks lane v < 16 holds m[v] and, only where
//          m[v] < gp[v], issues the global atomicMins into fnext[f[v]] and fnext[v]: fnext[f[v]] starts at gp[f[v]] <= gp[v], so a
//          larger m[v] cannot lower either word.  The returning form raises "changed" only where a word really fell, so
//          changed == 0 is exactly f' == f.  A line without entries in the walked orientations returns before its tile index is read.
//          No kernel plain-reads an array the same launch writes or hits with atomics: a round reads f and gp and mins into fnext,
//          the three buffers rotating; nothing waits on another workgroup.  The host reads the round's word back (4 bytes per round).
//   ids    components_roots_kernel: the flags label[v] == v; exclusive_scan_i32 turns them into ranks, its 64-bit total is the
//          number of components; components_ids_kernel: id[v] = rank[label[v]].
// The scratch is the graph routines' (pem_ctx::graph_scratch, carved by graph_carve): two buffers of n + 1 int32 -- with d_label the
// three the rounds rotate through; the first then holds the flags and ranks -- and the two round words of graph_rounds.
#include "spgemm_internal.h"
#include "tiled_internal.h"
#include "graph_internal.h"

using namespace pem;

namespace {

__global__ void __launch_bounds__(256) components_iota_kernel(int *__restrict__ f, const long long n)
{
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < n) f[v] = (int)v;
}

// gp = f[f], fnext = gp; *changed is raised where a grandparent is below the parent, *changed_next, the next round's word, is cleared
// (nobody else touches it in this round)
__global__ void __launch_bounds__(256) components_gp_kernel(const int *__restrict__ f, int *__restrict__ gp, int *__restrict__ fnext,
                                                            const long long n, int *changed, int *changed_next)
{
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v == 0) *changed_next = 0;
    if (v >= n) return;
    const int p = f[v], g = f[p];
    gp[v] = g;
    fnext[v] = g;
    if (g < p) *changed = 1;
}

// the hooks of one round: fnext (started as gp) takes m[v] at v and at f[v]; *changed is raised where a word fell
template <bool SYM>
__global__ void __launch_bounds__(256) components_hook_kernel(const GraphArgs g, const int *__restrict__ f, const int *__restrict__ gp, int *fnext,
                                                              int *changed)
{
    __shared__ int s_m[4 * 16];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long L = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (L >= g.nlines) return;   // (wave-uniform)
    bool any = g.R.lptr[L] < g.R.lptr[L + 1];
    if constexpr (!SYM) any = any || g.Cs.lptr[L] < g.Cs.lptr[L + 1];
    if (!any) return;   // (wave-uniform) no entry reaches this line: its words stay gp
    int *const m = s_m + wv * 16;
    if (lane < 16) m[lane] = INT_MAX;
    mx_wave_sync();
    // every entry's gp[far end] is folded into its near end's word of m (the wave's 16 words)
    auto entry = [&](const unsigned major, const long long j) { atomicMin(&m[major], gp[j]); };
    auto walk_on = [] { return false; };
    line_walk<false>(g.R, L, lane, entry, walk_on);
    if constexpr (!SYM) line_walk<true>(g.Cs, L, lane, entry, walk_on);
    mx_wave_sync();
    const long long v = 16 * L + lane;
    if (lane < 16 && v < g.n) {
        const int mv = m[lane];
        if (mv < gp[v]) {
            const int p = f[v];
            bool fell = atomicMin(&fnext[p], mv) > mv;
            if (p != (int)v) fell = (atomicMin(&fnext[v], mv) > mv) || fell;
            if (fell) *changed = 1;
        }
    }
}

__global__ void __launch_bounds__(256) components_roots_kernel(const int *__restrict__ label, const long long n, int *__restrict__ flag)
{
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < n) flag[v] = label[v] == (int)v ? 1 : 0;
}

__global__ void __launch_bounds__(256) components_ids_kernel(const int *__restrict__ label, const int *__restrict__ rank, const long long n,
                                                             int *__restrict__ id)
{
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < n) id[v] = rank[label[v]];
}

}  // namespace

extern "C" pem_status pem_tiled_components(pem_ctx *ctx, const pem_tiled *A, int symmetric, int32_t *d_label, int32_t *d_id,
                                           int64_t *ncomponents, int32_t *rounds)
{
    const char *fn = "pem_tiled_components";
    PEM_TRY(graph_enter(fn, ctx && A && d_label && ncomponents && rounds, A, "the components need", symmetric));
    const long long n = A->rows;
    if (Span(d_id, (size_t)n * 4).meets(Span(d_label, (size_t)n * 4))) {
        set_error("%s: d_id and d_label overlap", fn);
        return PEM_E_INVALID;
    }
    *ncomponents = 0;
    *rounds = 0;
    if (n == 0) return PEM_OK;
    PEM_ENTER(ctx);
    if (!symmetric) PEM_TRY(ensure_mx_cols(ctx, A));
    // two buffers of n + 1 words (the scan writes its total behind the ranks), then the two round words
    int *buf[3] = {d_label, nullptr, nullptr}, *words;
    PEM_TRY(graph_carve(ctx, {{&buf[1], (size_t)n + 1}, {&buf[2], (size_t)n + 1}, {&words, 2}}));
    const GraphArgs g = graph_args(A);
    const unsigned egrid = grid_for((size_t)n, 256);
    PEM_TRY(zero_flags(ctx));
    PEM_LAUNCH(ctx, components_iota_kernel, egrid, 256, buf[0], n);
    int r = 0, at = 0;   // f is buf[at]
    // a round reads f, writes gp and fnext (the other two); with both orientations walked f_t[v] <= the smallest vertex within
    // distance t of v, so only a false promise takes more than n rounds
    PEM_TRY(graph_rounds(
        ctx, fn, n, words, RoundPolicy{symmetric != 0, "%s: internal: the labels still changed in round %d of at most %lld"},
        [&](int, int *changed, int *changed_next) {
            int *const f = buf[at], *const gp = buf[(at + 1) % 3], *const fnext = buf[(at + 2) % 3];
            PEM_LAUNCH(ctx, components_gp_kernel, egrid, 256, f, gp, fnext, n, changed, changed_next);
            if (symmetric)
                PEM_LAUNCH_NAMED(ctx, "components_hook_kernel<rows>", (components_hook_kernel<true>), line_grid(g), 256, g, f, gp, fnext, changed);
            else
                PEM_LAUNCH_NAMED(ctx, "components_hook_kernel<both>", (components_hook_kernel<false>), line_grid(g), 256, g, f, gp, fnext, changed);
            at = (at + 2) % 3;
        },
        &r));
    if (at != 0) PEM_HIP(hipMemcpyAsync(d_label, buf[at], (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, ctx->stream));
    // the ids: flags and ranks in the first scratch buffer, in place
    int *const rank = buf[1];
    PEM_LAUNCH(ctx, components_roots_kernel, egrid, 256, d_label, n, rank);
    PEM_TRY(exclusive_scan_i32(ctx, rank, rank, (size_t)n, ctx->d_scalars));
    if (d_id) PEM_LAUNCH(ctx, components_ids_kernel, egrid, 256, d_label, rank, n, d_id);
    PEM_TRY(launch_status(ctx));
    int64_t total = 0;
    PEM_TRY(read_scalars(ctx, ctx->d_scalars, 1, &total));
    *ncomponents = total;
    *rounds = r;
    return PEM_OK;
}
