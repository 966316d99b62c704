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
//   hook   components_hook_kernel: the line walk of colour.hip -- one wave per line of 16 vertices, chunks of 64 entries,
//          chunk_tile_of, the (major, minor) byte -- over the row line and, unless the caller promised a symmetric pattern, over the
//          column line of the same 16 vertices (the column schedule of mxv.hip).  Every entry gathers gp[j] and mins it into its near
//          vertex's word of the wave's 16-word LDS area (LDS atomicMin).  After the walks lane v < 16 holds m[v] and, only where
//          m[v] < gp[v], issues the global atomicMins into fnext[f[v]] and fnext[v]: fnext[f[v]] starts at gp[f[v]] <= gp[v], so a
//          larger m[v] cannot lower either word.  The returning form raises "changed" only where a word really fell, so
//          changed == 0 is exactly f' == f.  A line without entries in the walked orientations returns before its tile index is read.
//          No kernel plain-reads an array the same launch writes or hits with atomics: a round reads f and gp and mins into fnext,
//          the three buffers rotating; nothing waits on another workgroup.  The host reads the round's word back (4 bytes per round).
//   ids    components_roots_kernel: the flags label[v] == v; exclusive_scan_i32 turns them into ranks, its 64-bit total is the
//          number of components; components_ids_kernel: id[v] = rank[label[v]].
// The scratch is the colouring's (pem_ctx::colour_scratch, grow-only; every call that uses it waits before it returns): two buffers
// of n + 1 int32 -- with d_label the three the rounds rotate through; the first then holds the flags and ranks -- and the two round
// words.
#include "spgemm_internal.h"
#include "tiled_internal.h"
#include "mx_internal.h"
#include <climits>

using namespace pem;

namespace {

// what a walk reads of one orientation of a tiling: the arguments of frontier_kernel
struct CompSide {
    const int *lptr, *poff, *pbase, *pminor;
    const uint8_t *rci;
};

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

// One orientation's walk for line L: every entry's gp[far end] is folded into its near end's word of m (the wave's 16 words).
template <bool COL>
__device__ __forceinline__ void components_walk(const CompSide &S, const long long L, const int lane, const int *__restrict__ gp, int *m)
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
            const long long j = 16 * (long long)t_minor + (rc & 15u);
            atomicMin(&m[rc >> 4], gp[j]);
        }
        // the next chunk starts in the tile of entry eb + 63, or in the one after it
        int pn = pc + ti_last;
        if (eb + 64 < e_end && pn + 1 < p1 && S.poff[pn + 1] <= eb + 64) ++pn;
        pc = pn;
    }
}

// the hooks of one round: fnext (started as gp) takes m[v] at v and at f[v]; *changed is raised where a word fell
template <bool SYM>
__global__ void __launch_bounds__(256) components_hook_kernel(const CompSide R, const CompSide Cs, const long long nlines, const long long n,
                                                              const int *__restrict__ f, const int *__restrict__ gp, int *fnext, int *changed)
{
    __shared__ int s_m[4 * 16];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long L = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (L >= nlines) return;   // (wave-uniform)
    bool any = R.lptr[L] < R.lptr[L + 1];
    if constexpr (!SYM) any = any || Cs.lptr[L] < Cs.lptr[L + 1];
    if (!any) return;   // (wave-uniform) no entry reaches this line: its words stay gp
    int *const m = s_m + wv * 16;
    if (lane < 16) m[lane] = INT_MAX;
    mx_wave_sync();
    components_walk<false>(R, L, lane, gp, m);
    if constexpr (!SYM) components_walk<true>(Cs, L, lane, gp, m);
    mx_wave_sync();
    const long long v = 16 * L + lane;
    if (lane < 16 && v < n) {
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
    if (!ctx || !A || !d_label || !ncomponents || !rounds) {
        set_error("%s: null argument", fn);
        return PEM_E_INVALID;
    }
    if (A->rows != A->cols) {
        set_error("%s: the tiling is %d x %d; the components need a square one", fn, A->rows, A->cols);
        return PEM_E_INVALID;
    }
    if (!fr_flag_ok(symmetric)) {
        set_error("%s: symmetric must be 0 or 1 (got %d)", fn, symmetric);
        return PEM_E_INVALID;
    }
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
    const size_t cbytes = (((size_t)n + 1) * sizeof(int) + 255) & ~size_t(255);
    PEM_TRY(ctx->colour_scratch.reserve(2 * cbytes + 256));
    char *const base = ctx->colour_scratch.as<char>();
    int *buf[3] = {d_label, reinterpret_cast<int *>(base), reinterpret_cast<int *>(base + cbytes)};
    int *const words = reinterpret_cast<int *>(base + 2 * cbytes);
    const CompSide R{A->tile_rowptr.as<int>(), A->tile_nnz_ptr.as<int>(), nullptr, A->tile_colidx.as<int>(), A->rowcolidx.as<uint8_t>()};
    const CompSide Cs{A->tile_colptr.as<int>(), A->mx_csc_off.as<int>(), A->mx_csc_base.as<int>(), A->tile_rowidx.as<int>(),
                      A->mx_rci_t.as<uint8_t>()};
    const long long nlines = A->tile_rows;
    const unsigned egrid = grid_for((size_t)n, 256), lgrid = grid_for((size_t)nlines * 64, 256);
    PEM_TRY(zero_flags(ctx));
    PEM_LAUNCH(ctx, components_iota_kernel, egrid, 256, buf[0], n);
    PEM_HIP(hipMemsetAsync(words, 0, 2 * sizeof(int), ctx->stream));
    int *const h_changed = reinterpret_cast<int *>(ctx->h_scalars);
    int r = 0, at = 0;   // f is buf[at]
    for (;;) {           // round r + 1 reads f, writes gp and fnext (the other two), raises words[r & 1] and clears the other word
        int *const f = buf[at], *const gp = buf[(at + 1) % 3], *const fnext = buf[(at + 2) % 3];
        int *const changed = words + (r & 1), *const changed_next = words + ((r + 1) & 1);
        PEM_LAUNCH(ctx, components_gp_kernel, egrid, 256, f, gp, fnext, n, changed, changed_next);
        if (symmetric)
            PEM_LAUNCH_NAMED(ctx, "components_hook_kernel<rows>", (components_hook_kernel<true>), lgrid, 256, R, Cs, nlines, n, f, gp, fnext, changed);
        else
            PEM_LAUNCH_NAMED(ctx, "components_hook_kernel<both>", (components_hook_kernel<false>), lgrid, 256, R, Cs, nlines, n, f, gp, fnext, changed);
        PEM_TRY(launch_status(ctx));
        PEM_HIP(hipMemcpyAsync(h_changed, changed, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        PEM_HIP(hipStreamSynchronize(ctx->stream));
        ++r;
        at = (at + 2) % 3;
        if (*h_changed == 0) break;
        if (r >= n) {   // (with both orientations walked f_t[v] <= the smallest vertex within distance t of v)
            if (symmetric) break;   // the promise was false
            set_error("%s: internal: the labels still changed in round %d of at most %lld", fn, r, n);
            return PEM_E_HIP;
        }
    }
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
