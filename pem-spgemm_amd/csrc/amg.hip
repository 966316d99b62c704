// amg.hip -- aggregation algebraic multigrid on a tiling (include/pem_spgemm.h, pem_amg_*): the hierarchy A_0 = A, P_l, R_l = P_l^T,
// A_{l+1} = R_l (A_l P_l), one V-cycle with weighted-Jacobi smoothing, and the refresh of every level's values on the patterns the
// setup found.
//
// The setup is a sequence of the library's own entry points, called as a user would call them -- pem_tiled_aggregate,
// pem_tiled_from_coo_device, pem_cplan_create + pem_spgemm + pem_tiled_from_cplan, pem_tiled_scale, pem_tiled_ewise,
// pem_tiled_transpose -- so every level is bit for bit what those calls give.  The refresh is step 3 of each plan followed by the
// matching pem_tiled_set_values_from_*.  What this file adds are the streaming kernels around them (kernel_stats names amg_*):
//   amg_weights    w_i = omega / d_i, d_i the stored (i, i) value, looked up in the diagonal tile; at create it also counts the rows
//                  without a stored diagonal entry
//   amg_triplets   the triplets of the tentative prolongator (row v, value 1; the column array is the aggregate array itself) and
//                  the count of vertices without an aggregate
//   amg_scale      x_i = w_i * b_i                      (a Jacobi sweep from x = 0)
//   amg_jacobi     x_i = x_i + w_i * (b_i - q_i)        (q = A x, pem_tiled_mxv's chain)
//   amg_residual   q_i = b_i - q_i                      (in place: every lane reads and writes its own element)
// The cycle's kernels hold no reduction and no atomic, one thread owns one element, and no kernel reads, at another index, an array
// its own launch writes: the bits do not depend on the launch shape.  The file is compiled with contraction off, so each product and
// each sum is rounded once.
//
// Launches of one pem_amg_apply (V = pem_amg_info::launches), s = sweeps, c = coarse_sweeps, the mxv launches included:
//   coarsest level     1 + 2 (c - 1)                                  amg_scale, then c - 1 times (mxv, amg_jacobi)
//   every other level  (1 + 2 (s - 1)) + 2 + 1 + 1 + 2 s = 4 s + 3    pre-smoothing; mxv, amg_residual; the restriction (mxv of R_l);
//                                                                     the prolongation (mxv of P_l, accumulate); post-smoothing
#include "spgemm_internal.h"
#include "tiled_internal.h"
#include "mx_internal.h"
#include <cmath>

using namespace pem;

namespace {

constexpr int AMG_THREADS = 256;

// w_i = omega / d_i; a row without a stored (i, i) gets omega / 0 and, with COUNT, is counted (count, and n - row as a maximum)
template <typename VT, bool COUNT>
__global__ void __launch_bounds__(AMG_THREADS) amg_weights_kernel(const long long n, const int *__restrict__ tile_rowptr,
                                                                   const int *__restrict__ tile_colidx, const int *__restrict__ tile_nnz_ptr,
                                                                   const uint32_t *__restrict__ tile_rec, const VT *__restrict__ vals,
                                                                   const VT omega, VT *__restrict__ w, unsigned long long *__restrict__ count,
                                                                   unsigned long long *__restrict__ first)
{
    const long long i = (long long)blockIdx.x * AMG_THREADS + threadIdx.x;
    if (i >= n) return;
    const int tr = (int)(i >> 4);
    const unsigned r = (unsigned)(i & 15);
    const int t = mask_find_tile(tile_rowptr, tile_colidx, tr, tr);
    VT d = VT(0);
    bool stored = false;
    if (t >= 0) {
        const uint32_t rec = tile_rec[16 * (size_t)t + r];
        if ((rec >> r) & 1u) {
            stored = true;
            d = vals[src_slot(tile_nnz_ptr[t], rec, r)];
        }
    }
    w[i] = omega / d;
    if constexpr (COUNT) {
        if (!stored) {
            atomicAdd(count, 1ull);
            atomicMax(first, (unsigned long long)(n - i));
        }
    }
}

// the tentative prolongator's triplets (v, agg[v], 1): rows and values here, the columns are agg; counts the agg[v] < 0
template <typename VT>
__global__ void __launch_bounds__(AMG_THREADS) amg_triplets_kernel(const long long n, const int *__restrict__ agg, int *__restrict__ rows,
                                                                    VT *__restrict__ ones, unsigned long long *__restrict__ unplaced)
{
    const long long v = (long long)blockIdx.x * AMG_THREADS + threadIdx.x;
    if (v >= n) return;
    rows[v] = (int)v;
    ones[v] = VT(1);
    if (agg[v] < 0) atomicAdd(unplaced, 1ull);
}

template <typename VT>
__global__ void __launch_bounds__(AMG_THREADS) amg_scale_kernel(const long long n, const VT *__restrict__ w, const VT *__restrict__ b,
                                                                 VT *__restrict__ x)
{
    const long long i = (long long)blockIdx.x * AMG_THREADS + threadIdx.x;
    if (i < n) x[i] = w[i] * b[i];
}

template <typename VT>
__global__ void __launch_bounds__(AMG_THREADS) amg_jacobi_kernel(const long long n, const VT *__restrict__ w, const VT *__restrict__ b,
                                                                  const VT *__restrict__ q, VT *__restrict__ x)
{
    const long long i = (long long)blockIdx.x * AMG_THREADS + threadIdx.x;
    if (i >= n) return;
    const VT t = b[i] - q[i];
    const VT u = w[i] * t;
    x[i] = x[i] + u;
}

template <typename VT>
__global__ void __launch_bounds__(AMG_THREADS) amg_residual_kernel(const long long n, const VT *__restrict__ b, VT *__restrict__ q)
{
    const long long i = (long long)blockIdx.x * AMG_THREADS + threadIdx.x;
    if (i < n) q[i] = b[i] - q[i];
}

struct Level {
    const pem_tiled *A = nullptr;       // level 0: the caller's handle; else A_next of the level above
    int64_t n = 0;
    int32_t rounds = 0;
    // what the level owns (null at the coarsest level; Pt, T, W, AP and the plans also after a create with refreshable = 0)
    pem_tiled *Pt = nullptr, *T = nullptr, *W = nullptr, *P = nullptr, *R = nullptr, *AP = nullptr, *A_next = nullptr;
    pem_cplan *planT = nullptr, *planAP = nullptr, *planRAP = nullptr;
    void *w = nullptr, *x = nullptr, *b = nullptr, *q = nullptr;   // into pem_amg::vec (level 0: x and b are the caller's)
};

}  // namespace

struct pem_amg {
    pem_ctx *owner = nullptr;
    const pem_tiled *A = nullptr;
    pem_amg_opts opts = {};
    int levels = 0;
    Level lv[PEM_AMG_MAX_LEVELS];
    DevBuf vec;          // every level's w, q and (below level 0) x, b: one block
    int64_t launches = 0, bytes = 0;
};

namespace {

void amg_free(pem_ctx *ctx, pem_amg *M, bool setup_only)
{
    for (int l = 0; l < PEM_AMG_MAX_LEVELS; ++l) {
        Level &L = M->lv[l];
        pem_cplan **plans[3] = {&L.planT, &L.planAP, &L.planRAP};
        for (pem_cplan **p : plans)
            if (*p) {
                pem_cplan_destroy(ctx, *p);
                *p = nullptr;
            }
        pem_tiled **mid[3] = {&L.T, &L.W, &L.AP};
        for (pem_tiled **t : mid)
            if (*t) {
                pem_tiled_destroy(ctx, *t);
                *t = nullptr;
            }
        if (L.Pt && L.Pt != L.P) pem_tiled_destroy(ctx, L.Pt);
        L.Pt = nullptr;
        if (setup_only) continue;
        pem_tiled **kept[3] = {&L.P, &L.R, &L.A_next};
        for (pem_tiled **t : kept)
            if (*t) {
                pem_tiled_destroy(ctx, *t);
                *t = nullptr;
            }
    }
}

struct AmgGuard {   // a failed create leaves nothing behind
    pem_ctx *ctx;
    pem_amg *M;
    ~AmgGuard()
    {
        if (M) {
            amg_free(ctx, M, false);
            delete M;
        }
    }
};

template <typename VT>
void launch_weights(pem_ctx *ctx, const pem_tiled *A, double omega, VT *w, unsigned long long *count)
{
    const long long n = A->rows;
    if (count)
        PEM_LAUNCH_NAMED(ctx, "amg_weights", (amg_weights_kernel<VT, true>), grid_for((size_t)n, AMG_THREADS), AMG_THREADS, n,
                         A->tile_rowptr.as<int>(), A->tile_colidx.as<int>(), A->tile_nnz_ptr.as<int>(), A->tile_rec.as<uint32_t>(),
                         A->vals.as<VT>(), (VT)omega, w, count, count + 1);
    else
        PEM_LAUNCH_NAMED(ctx, "amg_weights", (amg_weights_kernel<VT, false>), grid_for((size_t)n, AMG_THREADS), AMG_THREADS, n,
                         A->tile_rowptr.as<int>(), A->tile_colidx.as<int>(), A->tile_nnz_ptr.as<int>(), A->tile_rec.as<uint32_t>(),
                         A->vals.as<VT>(), (VT)omega, w, (unsigned long long *)nullptr, (unsigned long long *)nullptr);
}

// C = A B under plus_times with default options, as a plan and as a tiling
pem_status amg_product(pem_ctx *ctx, const pem_tiled *A, const pem_tiled *B, pem_cplan **plan, pem_tiled **C)
{
    PEM_TRY(pem_cplan_create(ctx, A, B, 0, -1, plan));
    PEM_TRY(pem_spgemm(ctx, *plan));
    return pem_tiled_from_cplan(ctx, *plan, 0, C);
}

// step 3 of a plan on its operands' new values and the values into the tiling made from it; stream-ordered
pem_status amg_reproduct(pem_ctx *ctx, pem_cplan *plan, pem_tiled *C)
{
    plan->warm_pass = false;
    PEM_TRY(step3_impl(ctx, plan));
    note_c_values(plan);
    return pem_tiled_set_values_from_cplan(ctx, C, plan);
}

template <typename VT>
pem_status amg_setup(pem_ctx *ctx, pem_amg *M)
{
    const char *fn = "pem_amg_create";
    const pem_amg_opts &o = M->opts;
    const size_t vb = sizeof(VT);
    DevBuf wtmp[PEM_AMG_MAX_LEVELS];   // the weights while the level sizes are not all known; copied into the one block at the end
    DevBuf agg, trip;
    unsigned long long *sc = reinterpret_cast<unsigned long long *>(ctx->d_scalars + 24);
    int l = 0;
    for (;; ++l) {
        Level &L = M->lv[l];
        L.n = L.A->rows;
        const long long n = L.n;
        M->levels = l + 1;
        if (n == 0) break;
        // the weights and the diagonal check
        if (L.A->ntiles == 0) {
            set_error("%s: level %d: row 1 has no stored diagonal entry (%lld such rows); the Jacobi smoother divides by it: store it", fn, l, n);
            return PEM_E_INVALID;
        }
        PEM_TRY(wtmp[l].reserve(n * vb));
        PEM_HIP(hipMemsetAsync(sc, 0, 2 * sizeof(int64_t), ctx->stream));
        launch_weights<VT>(ctx, L.A, o.omega, wtmp[l].as<VT>(), sc);
        int64_t got[2] = {0, 0};
        PEM_TRY(read_scalars(ctx, reinterpret_cast<const int64_t *>(sc), 2, got));
        PEM_TRY(launch_status(ctx));
        if (got[0]) {
            set_error("%s: level %d: row %lld has no stored diagonal entry (%lld such rows); the Jacobi smoother divides by it: store it", fn, l,
                      (long long)(n - got[1] + 1), (long long)got[0]);
            return PEM_E_INVALID;
        }
        if (l + 1 == o.max_levels || n <= o.coarse_size) break;
        // the aggregates
        PEM_TRY(agg.reserve(n * sizeof(int)));
        int64_t nc = 0;
        PEM_TRY(pem_tiled_aggregate(ctx, L.A, o.symmetric, o.seed, nullptr, agg.as<int32_t>(), nullptr, &nc, &L.rounds));
        if (nc == n) break;   // nothing coarsens
        // the tentative prolongator
        const size_t ibytes = ((size_t)n * sizeof(int) + 255) & ~size_t(255);
        PEM_TRY(trip.reserve(ibytes + n * vb));
        int *rows = trip.as<int>();
        VT *ones = reinterpret_cast<VT *>(trip.as<char>() + ibytes);
        PEM_HIP(hipMemsetAsync(sc + 2, 0, sizeof(int64_t), ctx->stream));
        PEM_LAUNCH_NAMED(ctx, "amg_triplets", (amg_triplets_kernel<VT>), grid_for((size_t)n, AMG_THREADS), AMG_THREADS, n,
                         (const int *)agg.as<int>(), rows, ones, sc + 2);
        int64_t unplaced = 0;
        PEM_TRY(read_scalars(ctx, reinterpret_cast<const int64_t *>(sc + 2), 1, &unplaced));
        PEM_TRY(launch_status(ctx));
        if (unplaced) {
            set_error("%s: level %d: %lld vertices have no aggregate: the pattern is not symmetric; pass symmetric = 0", fn, l,
                      (long long)unplaced);
            return PEM_E_INVALID;
        }
        if constexpr (sizeof(VT) == 8)
            PEM_TRY(pem_tiled_from_coo_device(ctx, (int)n, (int)nc, n, rows, agg.as<int32_t>(), ones, 0, &L.Pt));
        else
            PEM_TRY(pem_tiled_from_coo_device_f32(ctx, (int)n, (int)nc, n, rows, agg.as<int32_t>(), ones, 0, &L.Pt));
        // the prolongator
        if (o.smooth) {
            PEM_TRY(amg_product(ctx, L.A, L.Pt, &L.planT, &L.T));
            if constexpr (sizeof(VT) == 8)
                PEM_TRY(pem_tiled_scale(ctx, L.T, PEM_BINOP_TIMES, wtmp[l].as<VT>(), nullptr, &L.W));
            else
                PEM_TRY(pem_tiled_scale_f32(ctx, L.T, PEM_BINOP_TIMES, wtmp[l].as<VT>(), nullptr, &L.W));
            PEM_TRY(pem_tiled_ewise(ctx, L.Pt, L.W, PEM_EWISE_UNION, PEM_BINOP_PLUS, 1.0, -1.0, &L.P));
        } else {
            L.P = L.Pt;
        }
        // the coarse operator
        PEM_TRY(pem_tiled_transpose(ctx, L.P, &L.R));
        PEM_TRY(amg_product(ctx, L.A, L.P, &L.planAP, &L.AP));
        PEM_TRY(amg_product(ctx, L.R, L.AP, &L.planRAP, &L.A_next));
        M->lv[l + 1].A = L.A_next;
    }
    agg.release();
    trip.release();
    if (!o.refreshable) amg_free(ctx, M, true);
    // the work vectors of all levels in one block: w, q and, below level 0, x and b
    size_t total = 0;
    for (int k = 0; k < M->levels; ++k) total += (((size_t)M->lv[k].n * vb + 255) & ~size_t(255)) * (k ? 4 : 2);
    if (total) {
        PEM_TRY(M->vec.reserve(total));
        char *p = M->vec.as<char>();
        for (int k = 0; k < M->levels; ++k) {
            Level &L = M->lv[k];
            const size_t step = ((size_t)L.n * vb + 255) & ~size_t(255);
            L.w = p, p += step;
            L.q = p, p += step;
            if (k) {
                L.x = p, p += step;
                L.b = p, p += step;
            }
            if (L.n) PEM_HIP(hipMemcpyAsync(L.w, wtmp[k].p, (size_t)L.n * vb, hipMemcpyDeviceToDevice, ctx->stream));
        }
    }
    PEM_HIP(hipStreamSynchronize(ctx->stream));   // (wtmp goes back to the arena; create waits)
    M->launches = 0;
    for (int k = 0; k < M->levels; ++k) {
        if (!M->lv[k].n) continue;
        M->launches += k + 1 == M->levels ? 1 + 2 * ((int64_t)o.coarse_sweeps - 1) : 4 * (int64_t)o.sweeps + 3;
    }
    return PEM_OK;
}

template <typename VT>
pem_status amg_refresh(pem_ctx *ctx, pem_amg *M)
{
    for (int l = 0; l < M->levels; ++l) {
        Level &L = M->lv[l];
        if (!L.n) break;
        launch_weights<VT>(ctx, L.A, M->opts.omega, (VT *)L.w, nullptr);
        if (l + 1 == M->levels) break;
        if (M->opts.smooth) {
            PEM_TRY(amg_reproduct(ctx, L.planT, L.T));
            if constexpr (sizeof(VT) == 8)
                PEM_TRY(pem_tiled_set_values_from_scale(ctx, L.W, L.T, (const VT *)L.w, nullptr));
            else
                PEM_TRY(pem_tiled_set_values_from_scale_f32(ctx, L.W, L.T, (const VT *)L.w, nullptr));
            PEM_TRY(pem_tiled_set_values_from_ewise(ctx, L.P, L.Pt, L.W));
            PEM_TRY(pem_tiled_set_values_from_transpose(ctx, L.R, L.P));
        }
        PEM_TRY(amg_reproduct(ctx, L.planAP, L.AP));
        PEM_TRY(amg_reproduct(ctx, L.planRAP, L.A_next));
    }
    return PEM_OK;
}

template <typename VT>
struct Cycle {
    pem_ctx *ctx;
    pem_amg *M;

    static unsigned grid(long long n) { return grid_for((size_t)n, AMG_THREADS); }
    pem_status mxv(const pem_tiled *A, const VT *x, VT *y, int accumulate)
    {
        return mxv_semiring(ctx, A, PEM_SEMIRING_PLUS_TIMES, false, x, y, accumulate);
    }
    void scale(const Level &L, const VT *b, VT *x)
    {
        PEM_LAUNCH_NAMED(ctx, "amg_scale", (amg_scale_kernel<VT>), grid(L.n), AMG_THREADS, (long long)L.n, (const VT *)L.w, b, x);
    }
    pem_status sweeps(const Level &L, const VT *b, VT *x, int count)
    {
        for (int k = 0; k < count; ++k) {
            PEM_TRY(mxv(L.A, x, (VT *)L.q, 0));
            PEM_LAUNCH_NAMED(ctx, "amg_jacobi", (amg_jacobi_kernel<VT>), grid(L.n), AMG_THREADS, (long long)L.n, (const VT *)L.w, b,
                             (const VT *)L.q, x);
        }
        return PEM_OK;
    }
    pem_status run(int l, const VT *b, VT *x)
    {
        const Level &L = M->lv[l];
        const pem_amg_opts &o = M->opts;
        scale(L, b, x);
        if (l + 1 == M->levels) return sweeps(L, b, x, o.coarse_sweeps - 1);
        const Level &N = M->lv[l + 1];
        PEM_TRY(sweeps(L, b, x, o.sweeps - 1));
        PEM_TRY(mxv(L.A, x, (VT *)L.q, 0));
        PEM_LAUNCH_NAMED(ctx, "amg_residual", (amg_residual_kernel<VT>), grid(L.n), AMG_THREADS, (long long)L.n, b, (VT *)L.q);
        PEM_TRY(mxv(L.R, (const VT *)L.q, (VT *)N.b, 0));
        PEM_TRY(run(l + 1, (const VT *)N.b, (VT *)N.x));
        PEM_TRY(mxv(L.P, (const VT *)N.x, x, 1));
        return sweeps(L, b, x, o.sweeps);
    }
};

pem_status amg_apply(pem_ctx *ctx, pem_amg *M, const void *dr, void *dz, int value_bytes, const char *fn)
{
    if (!ctx || !M) {
        set_error("%s: null context or hierarchy", fn);
        return PEM_E_INVALID;
    }
    if (M->owner != ctx) {
        set_error("%s: the hierarchy was created on another context", fn);
        return PEM_E_INVALID;
    }
    if (M->A->value_bytes != value_bytes) {
        set_error("%s: the tiling holds %s values; use the %s entry point", fn, M->A->value_bytes == 4 ? "fp32" : "fp64",
                  M->A->value_bytes == 4 ? "_f32" : "fp64");
        return PEM_E_INVALID;
    }
    const size_t n = (size_t)M->A->rows;
    if (n == 0) return PEM_OK;
    if (!dr || !dz) {
        set_error("%s: null vector", fn);
        return PEM_E_INVALID;
    }
    if (Span(dr, n * value_bytes).meets(Span(dz, n * value_bytes))) {
        set_error("%s: d_r and d_z overlap", fn);
        return PEM_E_INVALID;
    }
    PEM_ENTER(ctx);
    if (value_bytes == 4) return Cycle<float>{ctx, M}.run(0, (const float *)dr, (float *)dz);
    return Cycle<double>{ctx, M}.run(0, (const double *)dr, (double *)dz);
}

}  // namespace

pem_ctx *pem::amg_owner(const pem_amg *M) { return M->owner; }
const pem_tiled *pem::amg_operator(const pem_amg *M) { return M->A; }

extern "C" pem_status pem_amg_create(pem_ctx *ctx, const pem_tiled *A, const pem_amg_opts *opts, pem_amg **out)
{
    const char *fn = "pem_amg_create";
    if (out) *out = nullptr;
    if (!ctx || !A || !opts || !out) {
        set_error("%s: null argument", fn);
        return PEM_E_INVALID;
    }
    if (A->rows != A->cols) {
        set_error("%s: the tiling is %d x %d; a multigrid hierarchy needs a square one", fn, A->rows, A->cols);
        return PEM_E_INVALID;
    }
    const pem_amg_opts &o = *opts;
    if ((o.smooth != 0 && o.smooth != 1) || (o.symmetric != 0 && o.symmetric != 1) || (o.refreshable != 0 && o.refreshable != 1)) {
        set_error("%s: smooth, symmetric and refreshable must be 0 or 1 (got %d, %d, %d)", fn, o.smooth, o.symmetric, o.refreshable);
        return PEM_E_INVALID;
    }
    if (o.max_levels < 1 || o.max_levels > PEM_AMG_MAX_LEVELS || o.coarse_size < 1 || o.sweeps < 1 || o.coarse_sweeps < 1) {
        set_error("%s: 1 <= max_levels <= %d, coarse_size >= 1, sweeps >= 1 and coarse_sweeps >= 1 are required (got %d, %lld, %d, %d)", fn,
                  (int)PEM_AMG_MAX_LEVELS, (int)o.max_levels, (long long)o.coarse_size, (int)o.sweeps, (int)o.coarse_sweeps);
        return PEM_E_INVALID;
    }
    if (!(o.omega > 0.0) || !std::isfinite(o.omega)) {
        set_error("%s: omega must be positive and finite (got %g)", fn, o.omega);
        return PEM_E_INVALID;
    }
    PEM_ENTER(ctx);
    const size_t before = ctx->arena->stats().in_use_bytes;
    AmgGuard G{ctx, new pem_amg};
    pem_amg *M = G.M;
    M->owner = ctx;
    M->A = A;
    M->opts = o;
    M->lv[0].A = A;
    PEM_TRY(A->value_bytes == 4 ? amg_setup<float>(ctx, M) : amg_setup<double>(ctx, M));
    const size_t after = ctx->arena->stats().in_use_bytes;
    M->bytes = after > before ? (int64_t)(after - before) : 0;
    G.M = nullptr;
    *out = M;
    return PEM_OK;
}

extern "C" pem_status pem_amg_refresh(pem_ctx *ctx, pem_amg *M)
{
    const char *fn = "pem_amg_refresh";
    if (!ctx || !M) {
        set_error("%s: null context or hierarchy", fn);
        return PEM_E_INVALID;
    }
    if (M->owner != ctx) {
        set_error("%s: the hierarchy was created on another context", fn);
        return PEM_E_INVALID;
    }
    if (!M->opts.refreshable) {
        set_error("%s: the hierarchy was created with refreshable = 0: its plans and intermediates are gone", fn);
        return PEM_E_STATE;
    }
    PEM_ENTER(ctx);
    return M->A->value_bytes == 4 ? amg_refresh<float>(ctx, M) : amg_refresh<double>(ctx, M);
}

extern "C" pem_status pem_amg_apply(pem_ctx *ctx, pem_amg *M, const double *d_r, double *d_z)
{
    return amg_apply(ctx, M, d_r, d_z, 8, "pem_amg_apply");
}

extern "C" pem_status pem_amg_apply_f32(pem_ctx *ctx, pem_amg *M, const float *d_r, float *d_z)
{
    return amg_apply(ctx, M, d_r, d_z, 4, "pem_amg_apply_f32");
}

extern "C" pem_status pem_amg_get_info(const pem_amg *M, pem_amg_info *info)
{
    if (!M || !info) {
        set_error("pem_amg_get_info: null argument");
        return PEM_E_INVALID;
    }
    *info = pem_amg_info{};
    info->levels = M->levels;
    for (int l = 0; l < M->levels; ++l) {
        const Level &L = M->lv[l];
        info->rows[l] = L.n;
        info->nnz[l] = L.A->nnz;
        info->p_nnz[l] = L.P ? L.P->nnz : 0;
        info->aggregate_rounds[l] = L.rounds;
    }
    info->launches = M->launches;
    info->bytes = M->bytes;
    return PEM_OK;
}

extern "C" pem_status pem_amg_get_level(const pem_amg *M, int level, const pem_tiled **A_l, const pem_tiled **P_l, const pem_tiled **R_l)
{
    if (!M || level < 0 || level >= M->levels) {
        set_error("pem_amg_get_level: null hierarchy, or level %d outside [0, %d)", level, M ? M->levels : 0);
        return PEM_E_INVALID;
    }
    const Level &L = M->lv[level];
    if (A_l) *A_l = L.A;
    if (P_l) *P_l = L.P;
    if (R_l) *R_l = L.R;
    return PEM_OK;
}

extern "C" pem_status pem_amg_destroy(pem_ctx *ctx, pem_amg *M)
{
    if (!M) return PEM_OK;
    amg_free(ctx ? ctx : M->owner, M, false);
    delete M;   // (a context's work is ordered on its stream: the arena may hand the blocks out again at once)
    return PEM_OK;
}
