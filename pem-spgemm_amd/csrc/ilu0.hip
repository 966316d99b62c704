// ilu0.hip -- incomplete LU of a square tiling on its own pattern (include/pem_spgemm.h, pem_tiled_ilu0): F has exactly A's
// pattern S and stores L's strict lower triangle (unit diagonal, not stored) and U with its diagonal.
//
// The order is the contract (m = min(i, j)), for every stored (i, j):
//   acc = a_ij; for k ascending over { k < m : (i, k) in S and (k, j) in S }: acc = fma(-f_ik, f_kj, acc);
//   f_ij = acc / f_jj where j < i (one IEEE division), else acc.
// A position that is not stored is never multiplied.  No atomics: the same bits on every call and on both launch routes.
//
// Dependencies at tile-row level are those of the lower solve -- tile row P waits for Q wherever tile (P, Q) is stored with
// Q < P -- so the schedule is the lower TrsvSched of the tiling itself (ensure_trsv, trsv.hip), and so are the launches: one per
// level wider than ILU0_MERGE tile rows, one single-workgroup launch per maximal run of narrower levels, a workgroup barrier with
// release/acquire fences between the levels of such a run.  No kernel waits on a value another workgroup writes in the same launch.
//
// One wave factors one tile row P.  All 64 lanes: lane = 4 i + g holds, of whatever tile it works on, row i's columns 4g .. 4g+3
// in registers (a row's 16 values are four lanes' consecutive loads) -- the same four positions of every tile, so a lane only
// ever reads back from F what it wrote itself; the values of other tile rows were written by earlier levels.  (The pointer is still not __restrict__, and a wavefront fence follows every
// write-back.)
//   phase 1   the lower tiles (P, Q) in ascending Q.  The diagonal tile (Q, Q) goes dense into the wave's LDS; for k = 0 .. 15 the
//             rows that store (i, k) divide by u_kk -- the quotient travels to the row's other three lanes by a shuffle -- and
//             apply fma(-l_ik, u_kj, .) to their stored (i, j), j > k, where (Q, Q) stores (k, j).  (P, Q) is written back and
//             stays in registers as L.  Then tile row Q's tiles (Q, R), R > Q, are merged against tile row P's sorted tile list
//             by two wave-uniform pointers (the shorter list is stepped through, the longer one searched by the whole wave): for
//             every R both hold, (Q, R) is staged in LDS, (P, R) is loaded, the same 16 steps run under mask_PR[i] & mask_QR[k],
//             and (P, R) is written back.  Q ascending and k ascending inside Q give every
//             entry its ascending-k chain, also in a lower tile (P, R) with Q < R < P: updated now, finished at its own turn.
//   phase 2   the diagonal tile (P, P) in 16 steps -- divide below the pivot, update to the right; row k's values come from its
//             lanes by shuffles -- then every upper tile (P, R): row i > k that stores (i, k) in the diagonal tile does
//             t[i][j] = fma(-l_ik, t[k][j], t[i][j]) on mask_PR[i] & mask_PR[k].
// LDS: one dense tile per wave (2 KiB in fp64), 32 KiB for the merged launch's 16 waves.
#include "spgemm_internal.h"
#include "tiled_internal.h"
#include "mx_internal.h"
#include <algorithm>

using namespace pem;

namespace {

constexpr int ILU0_MERGE = 16;   // merge_width: the waves of the merged launch's workgroup
constexpr int ILU0_WIDE = 4;     // waves per workgroup of a one-level launch

// ------------------------------------------------------------------------------------------
// a tile in a wave's registers: lane = 4 i + g holds row i's columns 4g .. 4g+3 (0 where not stored)
// ------------------------------------------------------------------------------------------
template <typename VT>
__device__ __forceinline__ void il_load(const VT *vals, const int off, const uint32_t rec, const int g, VT t[4])
{
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const unsigned j = 4u * g + c;
        t[c] = ((rec >> j) & 1u) ? vals[src_slot(off, rec, j)] : VT(0);
    }
}

// the write-back, then the wavefront fence every later read of F stands behind
template <typename VT>
__device__ __forceinline__ void il_store(VT *vals, const int off, const uint32_t rec, const int g, const VT t[4])
{
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const unsigned j = 4u * g + c;
        if ((rec >> j) & 1u) vals[src_slot(off, rec, j)] = t[c];
    }
    mx_wave_sync();
}

// a tile of an earlier tile row dense into the wave's LDS: s[16 r + c]; the slots of entries not stored are never read as values
// that count (every use is masked)
template <typename VT>
__device__ __forceinline__ void il_stage(VT *s, const VT *vals, const int off, const uint32_t rec, const int i, const int g)
{
    mx_wave_sync();   // the previous tile's steps have read the staging area
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const unsigned j = 4u * g + c;
        if ((rec >> j) & 1u) s[16 * i + j] = vals[src_slot(off, rec, j)];
    }
    mx_wave_sync();
}

// (P, Q) against the staged diagonal tile (Q, Q), whose row masks are rec_d (row r in the lanes 4r .. 4r+3): l becomes L's block
template <typename VT>
__device__ __forceinline__ void il_lower(VT l[4], const uint32_t rec_l, const uint32_t rec_d, const VT *s, const int i, const int g)
{
    const unsigned ml = rec_l & 0xFFFFu;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const bool has = (ml >> k) & 1u;
        if (g == (k >> 2) && has) l[k & 3] = l[k & 3] / s[17 * k];
        const VT lik = __shfl(l[k & 3], 4 * i + (k >> 2), 64);
        const unsigned m = ml & (unsigned)__shfl((int)rec_d, 4 * k, 64);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = 4 * g + c;
            if (has && j > k && ((m >> j) & 1u)) l[c] = pem_fma(-lik, s[16 * k + j], l[c]);
        }
    }
}

// (P, R) -= L(P, Q) * (Q, R): l the finished (P, Q), (Q, R) staged with its row masks rec_s
template <typename VT>
__device__ __forceinline__ void il_update(VT t[4], const uint32_t rec_t, const VT l[4], const uint32_t rec_l, const uint32_t rec_s, const VT *s,
                                          const int i, const int g)
{
    const unsigned ml = rec_l & 0xFFFFu, mt = rec_t & 0xFFFFu;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const bool has = (ml >> k) & 1u;
        const VT lik = __shfl(l[k & 3], 4 * i + (k >> 2), 64);
        const unsigned m = mt & (unsigned)__shfl((int)rec_s, 4 * k, 64);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = 4 * g + c;
            if (has && ((m >> j) & 1u)) t[c] = pem_fma(-lik, s[16 * k + j], t[c]);
        }
    }
}

// the diagonal tile (P, P) in place: row k is final when step k starts, and its values come from its lanes
template <typename VT>
__device__ __forceinline__ void il_diag(VT l[4], const uint32_t rec_l, const int i, const int g)
{
    const unsigned ml = rec_l & 0xFFFFu;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const bool has = i > k && ((ml >> k) & 1u);
        const VT ukk = __shfl(l[k & 3], 4 * k + (k >> 2), 64);
        if (g == (k >> 2) && has) l[k & 3] = l[k & 3] / ukk;
        const VT lik = __shfl(l[k & 3], 4 * i + (k >> 2), 64);
        const unsigned m = ml & (unsigned)__shfl((int)ml, 4 * k, 64);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = 4 * g + c;
            const VT u = __shfl(l[c], 4 * k + g, 64);
            if (has && j > k && ((m >> j) & 1u)) l[c] = pem_fma(-lik, u, l[c]);
        }
    }
}

// an upper tile (P, R) against the finished diagonal tile l: row k of the tile itself is final when step k starts
template <typename VT>
__device__ __forceinline__ void il_upper(VT t[4], const uint32_t rec_t, const VT l[4], const uint32_t rec_l, const int i, const int g)
{
    const unsigned ml = rec_l & 0xFFFFu, mt = rec_t & 0xFFFFu;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const bool has = i > k && ((ml >> k) & 1u);
        const VT lik = __shfl(l[k & 3], 4 * i + (k >> 2), 64);
        const unsigned m = mt & (unsigned)__shfl((int)mt, 4 * k, 64);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = 4 * g + c;
            const VT u = __shfl(t[c], 4 * k + g, 64);
            if (has && ((m >> j) & 1u)) t[c] = pem_fma(-lik, u, t[c]);
        }
    }
}

// the first position in [lo, hi) of the sorted tile list whose tile column is >= j (hi when there is none), searched by the whole
// wave: 64 evenly spaced probes and a ballot per round trip shrink the range 64-fold, where a binary search pays one dependent load
// per halving.  Every argument and the result are wave-uniform; all 64 lanes call it.
__device__ __forceinline__ int il_lower_bound(const int *__restrict__ colidx, int lo, int hi, const int j, const int lane)
{
    while (hi - lo > 64) {
        const int step = (hi - lo + 63) >> 6;
        const int pos = lo + lane * step;
        const int below = __popcll(__ballot(pos < hi && colidx[pos] < j));   // (sorted: the probes below j are the first `below`)
        if (below == 0) return lo;
        hi = min(hi, lo + below * step);
        lo += (below - 1) * step + 1;
    }
    const int pos = lo + lane;
    return lo + __popcll(__ballot(pos < hi && colidx[pos] < j));
}

// ------------------------------------------------------------------------------------------
// one wave, one tile row.  rows[P] = (first lower tile, end of the lower tiles, the diagonal tile or -1, level): the lower schedule
// ------------------------------------------------------------------------------------------
template <typename VT>
__device__ __forceinline__ void ilu0_tile_row(const int P, const int lane, VT *const my_s, const int4 *__restrict__ rows,
                                              const int *__restrict__ rowptr, const int *__restrict__ colidx, const int *__restrict__ poff,
                                              const uint32_t *__restrict__ tile_rec, VT *vals)
{
    const int i = lane >> 2, g = lane & 3;
    const int4 rw = rows[P];
    const int p1 = rw.y, dt = rw.z, pend = rowptr[P + 1];
    VT l[4], t[4];
    for (int p = rw.x; p < p1; ++p) {   // phase 1 (everything that steers it is wave-uniform)
        const int Q = colidx[p];
        const int dq = rows[Q].z;
        if (dq < 0) continue;   // (pem_tiled_ilu0 refuses a row without a stored diagonal entry)
        const uint32_t rec_l = tile_rec[16 * (size_t)p + i];
        const int off_l = poff[p];
        il_load(vals, off_l, rec_l, g, l);
        const uint32_t rec_d = tile_rec[16 * (size_t)dq + i];
        il_stage(my_s, vals, poff[dq], rec_d, i, g);
        il_lower(l, rec_l, rec_d, my_s, i, g);
        il_store(vals, off_l, rec_l, g, l);
        int a = dq + 1, b = p + 1;
        const int ae = rowptr[Q + 1];
        while (a < ae && b < pend) {   // step through the shorter list, search the longer one: a hub row meets short rows cheaply
            if (ae - a <= pend - b) {
                b = il_lower_bound(colidx, b, pend, colidx[a], lane);
                if (b < pend && colidx[b] != colidx[a]) ++a;
            } else {
                a = il_lower_bound(colidx, a, ae, colidx[b], lane);
                if (a < ae && colidx[a] != colidx[b]) ++b;
            }
            if (a >= ae || b >= pend || colidx[a] != colidx[b]) continue;
            const uint32_t rec_s = tile_rec[16 * (size_t)a + i], rec_t = tile_rec[16 * (size_t)b + i];
            const int off_t = poff[b];
            il_stage(my_s, vals, poff[a], rec_s, i, g);
            il_load(vals, off_t, rec_t, g, t);
            il_update(t, rec_t, l, rec_l, rec_s, my_s, i, g);
            il_store(vals, off_t, rec_t, g, t);
            ++a;
            ++b;
        }
    }
    if (dt < 0) return;   // phase 2
    const uint32_t rec_l = tile_rec[16 * (size_t)dt + i];
    const int off_l = poff[dt];
    il_load(vals, off_l, rec_l, g, l);
    il_diag(l, rec_l, i, g);
    il_store(vals, off_l, rec_l, g, l);
    for (int b = dt + 1; b < pend; ++b) {
        const uint32_t rec_t = tile_rec[16 * (size_t)b + i];
        const int off_t = poff[b];
        il_load(vals, off_t, rec_t, g, t);
        il_upper(t, rec_t, l, rec_l, i, g);
        il_store(vals, off_t, rec_t, g, t);
    }
}

// trsv_kernel's frame: order[lvl[v] .. lvl[v + 1]) are the tile rows of level v; the workgroup runs the levels [lv0, lv1) in order,
// wave w of the grid taking the w-th tile row of each; with more than one level the grid is one workgroup
template <typename VT, int WAVES>
__global__ void __launch_bounds__(64 * WAVES) ilu0_kernel(const int4 *__restrict__ rows, const int *__restrict__ order, const int *__restrict__ lvl,
                                                          const int lv0, const int lv1, const int *__restrict__ rowptr,
                                                          const int *__restrict__ colidx, const int *__restrict__ poff,
                                                          const uint32_t *__restrict__ tile_rec, VT *vals)
{
    __shared__ VT s_s[WAVES * 256];   // [wave][16 r + c]: the staged tile
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long w = (long long)blockIdx.x * WAVES + wv;
    for (int v = lv0; v < lv1; ++v) {   // (workgroup-uniform)
        const int w0 = lvl[v], width = lvl[v + 1] - w0;
        if (w < width)   // (wave-uniform)
            ilu0_tile_row<VT>(order[w0 + w], lane, s_s + wv * 256, rows, rowptr, colidx, poff, tile_rec, vals);
        if (v + 1 < lv1) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __syncthreads();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
    }
}

// vals_t[vmap_t[e]] = vals[e]: the column-major copy of the factor
template <typename VT>
__global__ void __launch_bounds__(256) ilu0_vals_t_kernel(const VT *__restrict__ vals, const int *__restrict__ map_t, const size_t nnz,
                                                          VT *__restrict__ vals_t)
{
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < nnz) vals_t[map_t[e]] = vals[e];
}

// the rows whose f_ii is +-0 or not finite: their count, and n - (the first of them) as a maximum (both start from 0)
template <typename VT>
__global__ void __launch_bounds__(256) ilu0_pivots_kernel(const int4 *__restrict__ rows, const int *__restrict__ poff,
                                                          const uint32_t *__restrict__ tile_rec, const VT *__restrict__ vals, const long long n,
                                                          unsigned long long *__restrict__ count, unsigned long long *__restrict__ first)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int dt = rows[i >> 4].z;
    const unsigned r = (unsigned)(i & 15);
    const uint32_t rec = dt >= 0 ? tile_rec[16 * (size_t)dt + r] : 0u;
    if ((rec >> r) & 1u) {   // (a diagonal entry that is not stored counts as a zero pivot)
        const VT d = vals[src_slot(poff[dt], rec, r)];
        if (d != VT(0) && d - d == VT(0)) return;   // (d - d is NaN for an infinite or NaN d)
    }
    atomicAdd(count, 1ull);
    atomicMax(first, (unsigned long long)(n - i));
}

int ilu0_merge_width(const pem_ctx *ctx) { return ctx->dbg_trsv_split ? 0 : ILU0_MERGE; }

// F's vals = A's vals, factored in place level by level, then vals_t.  F's lower schedule and vmap_t are ready.  Stream-ordered.
template <typename VT>
pem_status ilu0_launch(pem_ctx *ctx, const pem_tiled *A, pem_tiled *F)
{
    const TrsvSched &S = F->trsv[PEM_TRSV_LOWER];
    const size_t nnz = (size_t)F->nnz;
    PEM_HIP(hipMemcpyAsync(F->vals.p, A->vals.p, sizeof(VT) * nnz, hipMemcpyDeviceToDevice, ctx->stream));
    static const char *const names[2][2] = {{"ilu0_kernel<float,level>", "ilu0_kernel<float,merged>"},
                                            {"ilu0_kernel<double,level>", "ilu0_kernel<double,merged>"}};
    const int4 *rows = S.buf.as<int4>();
    const int *order = S.buf.as<int>() + S.order_off, *lvl = S.buf.as<int>() + S.lvl_off;
    trsv_for_launches(S, ilu0_merge_width(ctx), [&](int v, int e, bool merged) {
        const char *name = names[sizeof(VT) == 8][merged];
        if (merged) {
            PEM_LAUNCH_NAMED(ctx, name, (ilu0_kernel<VT, ILU0_MERGE>), 1, 64 * ILU0_MERGE, rows, order, lvl, v, e, F->tile_rowptr.as<int>(),
                             F->tile_colidx.as<int>(), F->tile_nnz_ptr.as<int>(), F->tile_rec.as<uint32_t>(), F->vals.as<VT>());
        } else {
            const size_t width = (size_t)(S.h_lvl[v + 1] - S.h_lvl[v]);
            PEM_LAUNCH_NAMED(ctx, name, (ilu0_kernel<VT, ILU0_WIDE>), grid_for(width, ILU0_WIDE), 64 * ILU0_WIDE, rows, order, lvl, v, e,
                             F->tile_rowptr.as<int>(), F->tile_colidx.as<int>(), F->tile_nnz_ptr.as<int>(), F->tile_rec.as<uint32_t>(),
                             F->vals.as<VT>());
        }
    });
    PEM_LAUNCH_NAMED(ctx, sizeof(VT) == 4 ? "ilu0_vals_t_kernel<float>" : "ilu0_vals_t_kernel<double>", ilu0_vals_t_kernel<VT>, grid_for(nnz, 256), 256,
                     F->vals.as<VT>(), F->vmap_t.as<int>(), nnz, F->vals_t.as<VT>());
    return PEM_OK;
}

pem_status ilu0_factor(pem_ctx *ctx, const pem_tiled *A, pem_tiled *F)
{
    if (!F->nnz) return PEM_OK;
    return F->value_bytes == 4 ? ilu0_launch<float>(ctx, A, F) : ilu0_launch<double>(ctx, A, F);
}

}  // namespace

extern "C" pem_status pem_tiled_ilu0(pem_ctx *ctx, const pem_tiled *A, pem_tiled **out)
{
    const char *fn = "pem_tiled_ilu0";
    if (out) *out = nullptr;
    if (!ctx || !A || !out) {
        set_error("%s: null context, operand or output", fn);
        return PEM_E_INVALID;
    }
    if (A->rows != A->cols) {
        set_error("%s: the tiling is %d x %d; an incomplete LU needs a square one", fn, A->rows, A->cols);
        return PEM_E_INVALID;
    }
    return build_derived(ctx, out, [&](pem_tiled *F) -> pem_status {
        F->derived.kind = Derivation::ILU0;
        F->derived.src[0] = A->serial;
        PEM_TRY(clone_structure(ctx, A, F, true));
        if (F->rows == 0) return PEM_OK;
        // F's own lower schedule: the factorisation's launch plan, the first solve's too; it counts the rows without a diagonal
        PEM_TRY(ensure_trsv(ctx, F, PEM_TRSV_LOWER));
        const TrsvSched &S = F->trsv[PEM_TRSV_LOWER];
        if (S.missing_diag) {
            set_error("%s: row %lld has no stored diagonal entry (%lld such rows); an incomplete LU needs every pivot stored", fn,
                      (long long)S.first_missing_row, (long long)S.missing_diag);
            return PEM_E_INVALID;
        }
        PEM_TRY(ensure_vmap_t(ctx, F));
        PEM_HIP(hipEventRecord(ctx->ev[6], ctx->stream));
        PEM_TRY(ilu0_factor(ctx, A, F));
        PEM_HIP(hipEventRecord(ctx->ev[7], ctx->stream));
        PEM_HIP(hipStreamSynchronize(ctx->stream));
        PEM_TRY(launch_status(ctx));
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ctx->ev[6], ctx->ev[7]) == hipSuccess) F->conv_tile_kernel_ms = ms;
        return PEM_OK;
    });
}

extern "C" pem_status pem_tiled_set_values_from_ilu0(pem_ctx *ctx, pem_tiled *F, const pem_tiled *A)
{
    const char *fn = "pem_tiled_set_values_from_ilu0";
    if (!ctx || !F || !A) {
        set_error("%s: null context, tiling or source", fn);
        return PEM_E_INVALID;
    }
    if (F->derived.kind != Derivation::ILU0 || F->derived.src[0] != A->serial) {
        set_error("%s: the tiling was not made by pem_tiled_ilu0 from this A", fn);
        return PEM_E_INVALID;
    }
    // (refresh_derived's body: vmap_t and the schedule are the build's, so nothing is allocated and nothing read back)
    if (F->nnz) {
        PEM_ENTER(ctx);
        PEM_TRY(ilu0_factor(ctx, A, F));
    }
    ++F->value_version;
    return PEM_OK;
}

extern "C" pem_status pem_tiled_ilu0_info(pem_ctx *ctx, const pem_tiled *F, pem_ilu0_info *out)
{
    const char *fn = "pem_tiled_ilu0_info";
    if (!ctx || !F || !out) {
        set_error("%s: null context, tiling or out", fn);
        return PEM_E_INVALID;
    }
    if (F->rows != F->cols) {
        set_error("%s: the tiling is %d x %d; an incomplete LU is square", fn, F->rows, F->cols);
        return PEM_E_INVALID;
    }
    *out = pem_ilu0_info{};
    out->merge_width = ilu0_merge_width(ctx);
    if (F->rows == 0) return PEM_OK;
    PEM_ENTER(ctx);
    PEM_TRY(ensure_trsv(ctx, F, PEM_TRSV_LOWER));   // (a factor made by pem_tiled_ilu0 has it from its build)
    const TrsvSched &S = F->trsv[PEM_TRSV_LOWER];
    out->levels = (int64_t)S.h_lvl.size() - 1;
    out->launches = trsv_for_launches(S, ilu0_merge_width(ctx), [](int, int, bool) {});
    out->max_width = S.max_width;
    int64_t *sc = ctx->d_scalars + 16;
    PEM_HIP(hipMemsetAsync(sc, 0, 2 * sizeof(int64_t), ctx->stream));
    const long long n = F->rows;
    if (F->value_bytes == 4)
        PEM_LAUNCH(ctx, ilu0_pivots_kernel<float>, grid_for((size_t)n, 256), 256, S.buf.as<int4>(), F->tile_nnz_ptr.as<int>(), F->tile_rec.as<uint32_t>(),
                   F->vals.as<float>(), n, reinterpret_cast<unsigned long long *>(sc), reinterpret_cast<unsigned long long *>(sc + 1));
    else
        PEM_LAUNCH(ctx, ilu0_pivots_kernel<double>, grid_for((size_t)n, 256), 256, S.buf.as<int4>(), F->tile_nnz_ptr.as<int>(), F->tile_rec.as<uint32_t>(),
                   F->vals.as<double>(), n, reinterpret_cast<unsigned long long *>(sc), reinterpret_cast<unsigned long long *>(sc + 1));
    int64_t got[2] = {0, 0};
    PEM_TRY(read_scalars(ctx, sc, 2, got));
    PEM_TRY(launch_status(ctx));
    out->zero_pivots = got[0];
    out->first_zero_pivot_row = got[0] ? (int64_t)F->rows - got[1] + 1 : 0;
    return PEM_OK;
}
