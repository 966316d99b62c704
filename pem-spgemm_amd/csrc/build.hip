// build.hip -- a tiling from triplets that may repeat a position (include/pem_spgemm.h, pem_tiled_build*), the duplicates folded on
// the device under a pem_binop, FIRST or SECOND, and the refresh of such a tiling from new triplet values
// (pem_tiled_set_values_from_build).  GraphBLAS's GrB_Matrix_build with a dup operator; pem_tiled_from_coo* refuses such input.
//
// The route is pem_tiled_from_coo's with one stage more.  The key (tile row | tile column | r | c) of every triplet and perm[e] = e
// (coo_sort_keys, convert.hip), then the stable radix sort: equal keys end up adjacent and, because the sort is stable and perm
// started as the identity, IN INPUT ORDER.  From there:
//   bd_heads_kernel    per sorted position: starts it a new entry (key != the key before), starts it a new tile.
//   pair scan          of both flag arrays: every position's output slot and tile, and the totals nnz and ntiles -- the one read-back of
//                      the route (pem_tiled_from_coo reads ntiles at the same point).
//   bd_compact_kernel  per sorted position that starts an entry: its (r << 4) | c byte, its run's first position (run_start), the
//                      tile-head scan over the ENTRIES (which is the positions' scan read at the entry heads) and, where it starts a
//                      tile, the tile key and first entry -- the sorted tile payload derive_tiled (convert.hip) starts from.
//   bd_gather_kernel   sv[e] = V[perm[e]]: the values in sorted order, the route's only uncoalesced access.  (Not for FIRST / SECOND.)
//   bd_fold_kernel     one lane per entry.  A run of at most inorder_max values is walked by its lane, strictly left to right.  The
//                      longer runs of a wave's 64 entries are then taken one after the other by the whole wave: 256 consecutive values
//                      per trip, four per lane folded left to right, the 64 partial results combined by a shuffle tree over ADJACENT
//                      lanes, the trips chained left to right -- the input order is regrouped, never reordered, and a million copies
//                      of one position are coalesced loads, not a million dependent ones in one lane.  The long runs are found by a
//                      ballot: no list, no counter, nothing waits for another wave.  FIRST and SECOND read V[perm[.]] at the run's
//                      first resp. last position.
//   derive_tiled       everything else.
// No float atomics: every value is produced by one lane (or one wave) in an order the input alone decides.
//
// Refresh (PEM_BUILD_KEEP_MAP): the tiling keeps perm and run_start; a refresh is bd_gather_kernel and bd_fold_kernel again -- the
// same kernels on the same schedule, so the same bits as a fresh build -- the fold writing vals and, through vmap_t, vals_t.
#include "spgemm_internal.h"
#include "tiled_internal.h"
#include <cstdlib>
#include <utility>

using namespace pem;

// ------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) bd_heads_kernel(const uint64_t *__restrict__ keys, size_t n, int *__restrict__ ehead, int *__restrict__ thead)
{
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const uint64_t k = keys[e];
    int eh = 1, th = 1;
    if (e > 0) {
        const uint64_t p = keys[e - 1];
        eh = k != p;
        th = (k >> 8) != (p >> 8);
    }
    ehead[e] = eh;
    thead[e] = th;
}

// ehx / thx = the exclusive scans of the entry / tile heads over the n sorted positions (n + 1 values each: ehx[n] = nnz, thx[n] =
// ntiles, the sizes the arrays written here were allocated from).  headx: the tile-head scan over the entries.
__global__ void __launch_bounds__(256) bd_compact_kernel(const uint64_t *__restrict__ keys, const int *__restrict__ ehx, const int *__restrict__ thx,
                                                         size_t n, int bits_tc, uint8_t *__restrict__ rowcolidx, int *__restrict__ headx,
                                                         int *__restrict__ run_start, long long *__restrict__ tile_keys,
                                                         int *__restrict__ tile_nnz_ptr)
{
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int s = ehx[e];
    if (ehx[e + 1] != s) {   // starts entry s
        const uint64_t k = keys[e];
        const int t = thx[e];
        rowcolidx[s] = (uint8_t)(k & 0xFF);
        headx[s] = t;
        run_start[s] = (int)e;
        if (thx[e + 1] != t) {   // ... and tile t
            const uint64_t tc = (k >> 8) & ((1ull << bits_tc) - 1ull);
            const uint64_t tr = k >> (8 + bits_tc);
            tile_keys[t] = (long long)((tr << 32) | tc);
            tile_nnz_ptr[t] = s;
        }
    }
    if (e == n - 1) {   // closing offsets
        const int nnz = ehx[n], nt = thx[n];
        tile_nnz_ptr[nt] = nnz;
        headx[nnz] = nt;
        run_start[nnz] = (int)n;
    }
}

template <typename VT>
__global__ void __launch_bounds__(256) bd_gather_kernel(const VT *__restrict__ V, const uint32_t *__restrict__ perm, size_t n, VT *__restrict__ sv)
{
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) sv[e] = V[perm[e]];
}

// one trip of the wave: x = the lane's partial result, lanes 0 .. lanes - 1 hold one.  Adjacent-lane tree: after the step of distance
// d, lane l (a multiple of 2d) holds the fold of lanes l .. l + 2d - 1 in order.  The result is lane 0's.
template <typename VT>
__device__ __forceinline__ VT bd_trip_tree(VT x, const int op, const int lane, const int lanes)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const VT y = __shfl_down(x, d, 64);
        if (lane + d < lanes) x = pem_binop_value<VT>(op, x, y);
    }
    return x;
}

// the whole wave folds sv[b .. e), e - b >= 1 (wave-uniform): trips of 256 consecutive values from b on, four per lane folded left
// to right, the 64 partial results by the tree, the trips chained left to right.  BD_AHEAD full trips are loaded before the first
// of them is folded (the chain would otherwise wait for memory once per trip); the grouping is the same either way.  The result
// is lane 0's.
constexpr int BD_AHEAD = 8;
template <typename VT>
__device__ __forceinline__ VT bd_wave_fold(const VT *__restrict__ sv, const int b, const int e, const int op, const int lane)
{
    VT acc = VT(0);
    long long base = b;   // (64 bits: e reaches INT32_MAX)
    while (base < e) {
        if (base + 256 * BD_AHEAD <= e) {
            VT v[BD_AHEAD][4];
#pragma unroll
            for (int u = 0; u < BD_AHEAD; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j) v[u][j] = sv[base + 256 * u + 4 * lane + j];
#pragma unroll
            for (int u = 0; u < BD_AHEAD; ++u) {
                VT x = pem_binop_value<VT>(op, v[u][0], v[u][1]);
                x = pem_binop_value<VT>(op, x, v[u][2]);
                x = bd_trip_tree<VT>(pem_binop_value<VT>(op, x, v[u][3]), op, lane, 64);
                acc = (base == b && u == 0) ? x : pem_binop_value<VT>(op, acc, x);
            }
            base += 256 * BD_AHEAD;
            continue;
        }
        const int cnt = e - base < 256 ? (int)(e - base) : 256;   // values of this trip
        const long long mine = base + 4 * lane;                   // the lane's four, in order
        const int nl = e - mine < 4 ? (int)(e - mine) : 4;        // (<= 0: none)
        VT x = VT(0);
        if (nl > 0) {
            x = sv[mine];
            for (int j = 1; j < nl; ++j) x = pem_binop_value<VT>(op, x, sv[mine + j]);
        }
        x = bd_trip_tree<VT>(x, op, lane, (cnt + 3) >> 2);
        acc = base == b ? x : pem_binop_value<VT>(op, acc, x);
        base += 256;
    }
    return acc;
}

// One lane per entry s: its run is the sorted positions run_start[s] .. run_start[s + 1] - 1.  sv: the values in sorted order (binops);
// V, perm: the input values and the permutation (FIRST / SECOND).  vmap_t != null (refresh): also vals_t[vmap_t[s]].
template <typename VT>
__global__ void __launch_bounds__(256) bd_fold_kernel(const VT *__restrict__ sv, const VT *__restrict__ V, const uint32_t *__restrict__ perm,
                                                      const int *__restrict__ run_start, size_t nnz, int op, int inorder_max,
                                                      const int *__restrict__ vmap_t, VT *__restrict__ vals, VT *__restrict__ vals_t)
{
    const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool live = s < nnz;   // (every lane of the wave takes part in the ballot and the shuffles below)
    const int b = live ? run_start[s] : 0, e = live ? run_start[s + 1] : 0;
    VT acc = VT(0);
    bool is_long = false;
    if (live) {
        if (op == PEM_DUP_FIRST) {
            acc = V[perm[b]];
        } else if (op == PEM_DUP_SECOND) {
            acc = V[perm[e - 1]];
        } else if (e - b <= inorder_max) {
            acc = sv[b];
            for (int i = b + 1; i < e; ++i) acc = pem_binop_value<VT>(op, acc, sv[i]);
        } else {
            is_long = true;
        }
    }
    unsigned long long todo = __ballot(is_long);
    while (todo) {   // (wave-uniform)
        const int src = __builtin_ctzll(todo);
        todo &= todo - 1ull;
        const int rb = __shfl(b, src, 64), re = __shfl(e, src, 64);
        const VT r = __shfl(bd_wave_fold<VT>(sv, rb, re, op, lane), 0, 64);
        if (lane == src) acc = r;
    }
    if (live) {
        vals[s] = acc;
        if (vmap_t) vals_t[vmap_t[s]] = acc;
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
// the longest run one lane walks, read when a tiling is BUILT (a refresh uses the value its build kept, so it groups every run as
// the build did whatever the environment says by then): PEM_BUILD_INORDER_MAX, or more under PEM_BUILD_INORDER (tools/build_pass.py measures the choice;
// never less, so the public fold-order contract holds whatever the environment says)
static int inorder_max()
{
    const char *env = getenv("PEM_BUILD_INORDER");
    const int v = env ? atoi(env) : 0;
    return v > PEM_BUILD_INORDER_MAX ? v : PEM_BUILD_INORDER_MAX;
}

static bool dup_known(int dup) { return (dup >= PEM_BINOP_PLUS && dup <= PEM_BINOP_LAND) || dup == PEM_DUP_FIRST || dup == PEM_DUP_SECOND; }

// gather + fold of n_in input values dV into vals (and vals_t where vmap_t is given); sv: n_in values of scratch
template <typename VT>
static void launch_fold(pem_ctx *ctx, const void *dV, const uint32_t *perm, size_t n_in, const int *run_start, size_t nnz, int dup, int threshold, void *sv,
                        const int *vmap_t, void *vals, void *vals_t)
{
    const bool pick = dup == PEM_DUP_FIRST || dup == PEM_DUP_SECOND;
    if (!pick)
        PEM_LAUNCH(ctx, bd_gather_kernel<VT>, grid_for(n_in, 256), 256, static_cast<const VT *>(dV), perm, n_in, static_cast<VT *>(sv));
    PEM_LAUNCH(ctx, bd_fold_kernel<VT>, grid_for(nnz, 256), 256, static_cast<const VT *>(sv), static_cast<const VT *>(dV), perm, run_start, nnz, dup,
               threshold, vmap_t, static_cast<VT *>(vals), static_cast<VT *>(vals_t));
}

static void swap_bufs(DevBuf &a, DevBuf &b)
{
    std::swap(a.p, b.p);
    std::swap(a.cap, b.cap);
    std::swap(a.arena, b.arena);
}

static pem_status build_route(pem_ctx *ctx, pem_tiled *T, int rows, int cols, size_t n, const int *dI, const int *dJ, const void *dV,
                              int value_bytes, int transpose, int dup, int flags)
{
    set_tiled_shape(T, value_bytes, transpose ? cols : rows, transpose ? rows : cols);
    const int bits_tr = bits_for((uint64_t)T->tile_rows), bits_tc = bits_for((uint64_t)T->tile_cols);
    const bool pick = dup == PEM_DUP_FIRST || dup == PEM_DUP_SECOND;
    const int threshold = inorder_max();
    // every buffer sized by the triplets is local and goes back to the arena with the call, but for what PEM_BUILD_KEEP_MAP keeps
    DevBuf k0, k1, v0, v1, ehx, thx, sv, rs_tmp;
    PEM_TRY(zero_flags(ctx));
    PEM_TRY(arena_phase(ctx->arena, {{&k0, sizeof(uint64_t) * (n + 1)}, {&k1, sizeof(uint64_t) * (n + 1)}, {&v0, sizeof(uint32_t) * (n + 1)},
                                     {&v1, sizeof(uint32_t) * (n + 1)}, {&ehx, sizeof(int) * (n + 4)}, {&thx, sizeof(int) * (n + 4)},
                                     {&sv, pick ? 0 : (size_t)value_bytes * (n + 1)},
                                     {&ctx->sort_hist, sizeof(int) * (256 * (n / 4096 + 1) + 4)}}));
    PEM_TRY(k0.reserve(sizeof(uint64_t) * (n + 1)));
    PEM_TRY(k1.reserve(sizeof(uint64_t) * (n + 1)));
    PEM_TRY(v0.reserve(sizeof(uint32_t) * (n + 1)));
    PEM_TRY(v1.reserve(sizeof(uint32_t) * (n + 1)));
    PEM_TRY(ehx.reserve(sizeof(int) * (n + 4)));
    PEM_TRY(thx.reserve(sizeof(int) * (n + 4)));
    if (n) coo_sort_keys(ctx, T, dI, dJ, n, transpose, bits_tc, k0.as<uint64_t>(), v0.as<uint32_t>());
    uint64_t *keys = k0.as<uint64_t>();
    uint32_t *perm = v0.as<uint32_t>();
    PEM_TRY(radix_sort_u64_u32(ctx, k0.as<uint64_t>(), k1.as<uint64_t>(), v0.as<uint32_t>(), v1.as<uint32_t>(), n, 8 + bits_tc + bits_tr, &keys, &perm));
    if (n) PEM_LAUNCH(ctx, bd_heads_kernel, grid_for(n, 256), 256, keys, n, ehx.as<int>(), thx.as<int>());
    PEM_TRY(exclusive_scan_i32_pair(ctx, ehx.as<int>(), thx.as<int>(), n, ctx->d_scalars, ctx->d_scalars + 1));
    int64_t tot[2] = {0, 0};
    PEM_TRY(read_scalars(ctx, ctx->d_scalars, 2, tot));
    int hf[NUM_FLAGS];
    PEM_TRY(read_flags(ctx, hf));
    PEM_TRY(check_internal(hf));   // (a scan gave up: the sizes and every offset behind them would be wrong)
    if (hf[FLAG_RANGE]) {
        set_error("index out of range for a %d x %d matrix", T->rows, T->cols);
        return PEM_E_INVALID;
    }
    if (tot[0] < 0 || tot[0] > (int64_t)n || tot[1] < 0 || tot[1] > tot[0]) {
        set_error("pem_tiled_build: internal: %lld entries in %lld tiles from %lld triplets", (long long)tot[0], (long long)tot[1], (long long)n);
        return PEM_E_HIP;
    }
    T->nnz = tot[0];
    T->ntiles = tot[1];
    const size_t nnz = (size_t)T->nnz;
    const bool keep = (flags & PEM_BUILD_KEEP_MAP) != 0;
    DevBuf &rs = keep ? T->derived.idx[0] : rs_tmp;
    PEM_TRY(reserve_payload(ctx, T));
    PEM_TRY(rs.reserve(sizeof(int) * (nnz + 4)));
    if (!pick) PEM_TRY(sv.reserve((size_t)value_bytes * (n + 1)));
    int *headx;
    PEM_TRY(begin_payload(ctx, T, &headx));
    if (n) {
        PEM_LAUNCH(ctx, bd_compact_kernel, grid_for(n, 256), 256, keys, ehx.as<int>(), thx.as<int>(), n, bits_tc, T->rowcolidx.as<uint8_t>(), headx,
                   rs.as<int>(), T->tile_keys.as<long long>(), T->tile_nnz_ptr.as<int>());
        if (value_bytes == 4)
            launch_fold<float>(ctx, dV, perm, n, rs.as<int>(), nnz, dup, threshold, sv.p, nullptr, T->vals.p, nullptr);
        else
            launch_fold<double>(ctx, dV, perm, n, rs.as<int>(), nnz, dup, threshold, sv.p, nullptr, T->vals.p, nullptr);
    }
    PEM_TRY(derive_tiled(ctx, T, headx, bits_tr, bits_tc));   // (synchronises: the temporaries may go)
    if (keep) {
        Derivation &d = T->derived;
        d.kind = Derivation::BUILD;
        d.op = dup;
        d.pattern = threshold;
        d.p0 = (double)n;
        swap_bufs(d.map, perm == v0.as<uint32_t>() ? v0 : v1);   // the sort's permutation, where the sort left it
        d.map_ready = true;
    }
    return PEM_OK;
}

static pem_status build_device(pem_ctx *ctx, int rows, int cols, int64_t nnz_in, const int *dI, const int *dJ, const void *dV, int value_bytes,
                               int transpose, int dup, int flags, pem_tiled **out, const char *fn)
{
    if (out) *out = nullptr;
    if (!ctx || !out || rows <= 0 || cols <= 0 || nnz_in < 0) {
        set_error("%s: bad arguments (rows=%d cols=%d nnz_in=%lld)", fn, rows, cols, (long long)nnz_in);
        return PEM_E_INVALID;
    }
    if (!dup_known(dup)) {
        set_error("%s: unknown op %d (a pem_binop 0 .. 5, PEM_DUP_FIRST = 6 or PEM_DUP_SECOND = 7)", fn, dup);
        return PEM_E_INVALID;
    }
    if (flags & ~PEM_BUILD_KEEP_MAP) {
        set_error("%s: unknown flags %d (0 or PEM_BUILD_KEEP_MAP = 1)", fn, flags);
        return PEM_E_INVALID;
    }
    if (nnz_in > 0x7FFFFFFFll) {
        set_error("nnz=%lld exceeds the reference's int32 index range", (long long)nnz_in);
        return PEM_E_OVERFLOW;
    }
    if (nnz_in > 0 && (!dI || !dJ || !dV)) {
        set_error("%s: null triplet arrays for nnz_in=%lld", fn, (long long)nnz_in);
        return PEM_E_INVALID;
    }
    return build_derived(ctx, out, [&](pem_tiled *T) {
        pem_status s = build_route(ctx, T, rows, cols, (size_t)nnz_in, dI, dJ, dV, value_bytes, transpose, dup, flags);
        (void)hipStreamSynchronize(ctx->stream);   // (the temporaries went back to the arena)
        return s;
    });
}

static pem_status build_host(pem_ctx *ctx, int rows, int cols, int64_t nnz_in, const int32_t *I, const int32_t *J, const void *V, int value_bytes,
                             int transpose, int dup, int flags, pem_tiled **out, const char *fn)
{
    if (out) *out = nullptr;
    if (!ctx || !out || nnz_in < 0 || nnz_in > 0x7FFFFFFFll || (nnz_in > 0 && (!I || !J || !V)))   // (the device form words the refusal)
        return build_device(ctx, rows, cols, nnz_in, nullptr, nullptr, nullptr, value_bytes, transpose, dup, flags, out, fn);
    PEM_ENTER(ctx);
    DevBuf dI, dJ, dV;
    const size_t n = (size_t)nnz_in;
    PEM_TRY(dI.reserve(sizeof(int) * (n + 1)));
    PEM_TRY(dJ.reserve(sizeof(int) * (n + 1)));
    PEM_TRY(dV.reserve((size_t)value_bytes * (n + 1)));
    if (n) {
        PEM_HIP(hipMemcpyAsync(dI.p, I, sizeof(int) * n, hipMemcpyHostToDevice, ctx->stream));
        PEM_HIP(hipMemcpyAsync(dJ.p, J, sizeof(int) * n, hipMemcpyHostToDevice, ctx->stream));
        PEM_HIP(hipMemcpyAsync(dV.p, V, (size_t)value_bytes * n, hipMemcpyHostToDevice, ctx->stream));
    }
    pem_status s = build_device(ctx, rows, cols, nnz_in, dI.as<int>(), dJ.as<int>(), dV.p, value_bytes, transpose, dup, flags, out, fn);
    (void)hipStreamSynchronize(ctx->stream);
    return s;
}

extern "C" pem_status pem_tiled_build(pem_ctx *ctx, int rows, int cols, int64_t nnz_in, const int32_t *I, const int32_t *J, const double *V,
                                      int transpose, int dup, int flags, pem_tiled **out)
{
    return build_host(ctx, rows, cols, nnz_in, I, J, V, 8, transpose, dup, flags, out, "pem_tiled_build");
}
extern "C" pem_status pem_tiled_build_f32(pem_ctx *ctx, int rows, int cols, int64_t nnz_in, const int32_t *I, const int32_t *J, const float *V,
                                          int transpose, int dup, int flags, pem_tiled **out)
{
    return build_host(ctx, rows, cols, nnz_in, I, J, V, 4, transpose, dup, flags, out, "pem_tiled_build_f32");
}
extern "C" pem_status pem_tiled_build_device(pem_ctx *ctx, int rows, int cols, int64_t nnz_in, const int32_t *dI, const int32_t *dJ,
                                             const double *dV, int transpose, int dup, int flags, pem_tiled **out)
{
    return build_device(ctx, rows, cols, nnz_in, dI, dJ, dV, 8, transpose, dup, flags, out, "pem_tiled_build_device");
}
extern "C" pem_status pem_tiled_build_device_f32(pem_ctx *ctx, int rows, int cols, int64_t nnz_in, const int32_t *dI, const int32_t *dJ,
                                                 const float *dV, int transpose, int dup, int flags, pem_tiled **out)
{
    return build_device(ctx, rows, cols, nnz_in, dI, dJ, dV, 4, transpose, dup, flags, out, "pem_tiled_build_device_f32");
}

static pem_status refresh_from_build(pem_ctx *ctx, pem_tiled *t, const void *dV, int64_t nnz_in, int value_bytes, const char *fn)
{
    if (!ctx || !t) {
        set_error("%s: null context or tiling", fn);
        return PEM_E_INVALID;
    }
    const Derivation &d = t->derived;
    if (d.kind != Derivation::BUILD) {
        set_error("%s: the tiling was not made by pem_tiled_build with PEM_BUILD_KEEP_MAP", fn);
        return PEM_E_INVALID;
    }
    if ((double)nnz_in != d.p0) {
        set_error("%s: the tiling was not made by pem_tiled_build with PEM_BUILD_KEEP_MAP from %lld triplets", fn, (long long)nnz_in);
        return PEM_E_INVALID;
    }
    if (t->value_bytes != value_bytes) {
        set_error("%s: the tiling holds %s values; use the %s entry points", fn, t->value_bytes == 4 ? "fp32" : "fp64",
                  t->value_bytes == 4 ? "_f32" : "fp64");
        return PEM_E_INVALID;
    }
    if (nnz_in > 0 && !dV) {
        set_error("%s: null values for %lld triplets", fn, (long long)nnz_in);
        return PEM_E_INVALID;
    }
    const size_t n = (size_t)nnz_in, nnz = (size_t)t->nnz;
    const bool pick = d.op == PEM_DUP_FIRST || d.op == PEM_DUP_SECOND;
    PEM_ENTER(ctx);
    DevBuf &sv = ctx->tmp[1];   // the values in sorted order; context-owned, grow-only: a repeat refresh allocates nothing
    if (nnz && !pick) PEM_TRY(sv.reserve((size_t)value_bytes * (n + 1)));
    return refresh_derived(
        ctx, t, [] { return PEM_OK; },   // (the map is the build's)
        [&] {
            if (value_bytes == 4)
                launch_fold<float>(ctx, dV, d.map.as<uint32_t>(), n, d.idx[0].as<int>(), nnz, d.op, d.pattern, sv.p, t->vmap_t.as<int>(), t->vals.p, t->vals_t.p);
            else
                launch_fold<double>(ctx, dV, d.map.as<uint32_t>(), n, d.idx[0].as<int>(), nnz, d.op, d.pattern, sv.p, t->vmap_t.as<int>(), t->vals.p, t->vals_t.p);
        });
}

extern "C" pem_status pem_tiled_set_values_from_build(pem_ctx *ctx, pem_tiled *t, const double *dV, int64_t nnz_in)
{
    return refresh_from_build(ctx, t, dV, nnz_in, 8, "pem_tiled_set_values_from_build");
}
extern "C" pem_status pem_tiled_set_values_from_build_f32(pem_ctx *ctx, pem_tiled *t, const float *dV, int64_t nnz_in)
{
    return refresh_from_build(ctx, t, dV, nnz_in, 4, "pem_tiled_set_values_from_build_f32");
}
