// trsv.hip -- triangular solve on a tiling's lower or upper triangle (include/pem_spgemm.h, pem_tiled_trsv): x = T^-1 b, T the
// chosen triangle of a square tiling as stored; the other side is ignored, and under unit_diag so is the stored diagonal.
//
// The order is the contract (P = i / 16):
//   lower, rows ascending   acc = b_i; the stored a_ij with j < i in ascending j: acc = fma(-a_ij, x_j, acc); x_i = acc / a_ii.
//   upper, rows descending  acc = b_i; the stored a_ij with j >= 16 (P + 1) in ascending j, then those with i < j < 16 (P + 1) in
//                           descending j, the same fma; then the division.
// A recurrence, not a fold, so it runs by a schedule kept with the tiling (TrsvSched, pem_internal.h): tile row P waits for tile
// row Q wherever tile (P, Q) is stored on the chosen side, level(P) = 1 + the largest level it waits for, and the tile rows are
// listed by level.  The schedule is built on the HOST from tile_rowptr and tile_colidx (two int arrays read back once per
// pattern and triangle, no entry-level data); the rows without a stored diagonal entry are counted on the device from the
// diagonal tiles' tile_rec masks.
// One wave solves one tile row, acc of row 16 P + r in lane r:
//   phase 1   mxv's line walk (mxv.hip) over the row's off-diagonal tiles on the chosen side -- shuffle search, 16 ballots, LDS
//             staging of (a, x), the chain four reads ahead -- started from b and stepping fma(-a, x, acc).  These x belong to
//             tile rows of earlier levels.
//   phase 2   the diagonal tile, staged (column-major, dense) in the wave's own LDS before phase 1 starts: 16 steps, lane c
//             divides, x_c goes to every lane, the lanes whose row stores (r, c) on the chosen side do their fma.
// Levels wider than TRSV_MERGE tile rows are one launch each (four waves per workgroup); a maximal run of narrower levels is ONE
// launch of one workgroup of TRSV_MERGE waves that runs the levels in order with a workgroup barrier and fence between them.
// No kernel waits on a value another workgroup writes in the same launch: every cross-workgroup dependency is a kernel boundary.
// No atomics in the solve.  x and b may be the same array: neither is __restrict__, and a lane reads b_i before row i is written.
#include "spgemm_internal.h"
#include "tiled_internal.h"
#include "mx_internal.h"
#include <algorithm>
#include <climits>

using namespace pem;

namespace {

constexpr int TRSV_MERGE = 16;   // merge_width: the waves of the merged launch's workgroup
constexpr int TRSV_WIDE = 4;     // waves per workgroup of a one-level launch

// ------------------------------------------------------------------------------------------
// one wave, one tile row
// ------------------------------------------------------------------------------------------
template <typename VT, bool UPPER>
__device__ __forceinline__ void trsv_tile_row(const int P, const int lane, VT *const my_t, VT *const my_x, VT *const my_d, const int4 *__restrict__ rows,
                                              const int *__restrict__ poff, const int *__restrict__ pminor, const uint8_t *__restrict__ rci,
                                              const uint32_t *__restrict__ tile_rec, const VT *__restrict__ vals, const VT *b, VT *x,
                                              const long long n, const int unit)
{
    const int4 rw = rows[P];
    const int p0 = rw.x, p1 = rw.y, dt = rw.z;
    const long long o = 16LL * P + lane;
    const bool out_lane = lane < 16 && o < n;
    VT acc = out_lane ? b[o] : VT(0);
    // the diagonal tile, dense and column-major: my_d[16 c + r]; the slots of entries not stored are never used (dmask)
    unsigned dmask = 0;
    if (dt >= 0) {   // (wave-uniform)
        if (lane < 16) dmask = tile_rec[16 * (size_t)dt + lane] & 0xFFFFu;
        const int d0 = poff[dt], dn = poff[dt + 1] - d0;
        mx_wave_sync();   // the wave's previous tile row has read the dense tile
        for (int k = lane; k < dn; k += 64) {
            const unsigned rc = rci[d0 + k];
            my_d[16 * (rc & 15u) + (rc >> 4)] = vals[d0 + k];
        }
    }
    // phase 1: the line walk of mxv_kernel over the positions [p0, p1)
    if (p0 < p1) {
        const int e_end = poff[p1];
        int pc = p0;   // the tile holding the chunk's first entry (wave-uniform)
        for (int eb = poff[p0]; eb < e_end; eb += 64) {   // wave-uniform trip count
            const int mp = pc + lane;
            const bool lv = mp < p1;
            const int my_off = lv ? poff[mp] : INT_MAX;
            const int my_minor = lv ? pminor[mp] : 0;
            const int e = eb + lane;
            const int ti = chunk_tile_of(my_off, e);
            const int t_minor = __shfl(my_minor, ti, 64);
            const int ti_last = __shfl(ti, 63, 64);
            int major = 16;
            VT a = VT(0), xv = VT(0);
            if (e < e_end) {
                const unsigned rc = rci[e];
                major = (int)(rc >> 4);
                a = vals[e];
                xv = x[16 * (size_t)t_minor + (rc & 15u)];
            }
            // regroup the chunk by row: slot = entries of smaller rows + entries of the same row in lower lanes
            int slot = 0, my_first = 0, my_cnt = 0, run = 0;
#pragma unroll
            for (int m = 0; m < 16; ++m) {
                const unsigned long long bl = __ballot(major == m);
                const int cnt = __popcll(bl);
                if (major == m) slot = run + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bl >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bl, 0u));
                if (lane == m) {
                    my_first = run;
                    my_cnt = cnt;
                }
                run += cnt;
            }
            mx_wave_sync();   // the previous chunk's chain has read the staging area
            if (major < 16) {
                my_t[slot] = a;
                my_x[slot] = xv;
            }
            mx_wave_sync();
            const VT *pt = my_t + my_first;
            const VT *px = my_x + my_first;
            int k = 0;
            for (; k + 4 <= my_cnt; k += 4) {   // four reads ahead of the chain
                const VT t0 = pt[k], t1 = pt[k + 1], t2 = pt[k + 2], t3 = pt[k + 3];
                const VT x0 = px[k], x1 = px[k + 1], x2 = px[k + 2], x3 = px[k + 3];
                acc = pem_fma(-t0, x0, acc);
                acc = pem_fma(-t1, x1, acc);
                acc = pem_fma(-t2, x2, acc);
                acc = pem_fma(-t3, x3, acc);
            }
            for (; k < my_cnt; ++k) acc = pem_fma(-pt[k], px[k], acc);
            // the next chunk starts in the tile of entry eb + 63, or in the one after it
            int pn = pc + ti_last;
            if (eb + 64 < e_end && pn + 1 < p1 && poff[pn + 1] <= eb + 64) ++pn;
            pc = pn;
        }
    }
    // phase 2: substitution inside the diagonal tile
    if (dt >= 0) {
        mx_wave_sync();   // the dense tile is staged
        VT dv[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) dv[c] = lane < 16 ? my_d[16 * c + lane] : VT(0);
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int c = UPPER ? 15 - s : s;
            if (lane == c && out_lane && !unit) acc = acc / dv[c];
            const VT xc = __shfl(acc, c, 64);
            const bool side = UPPER ? lane < c : lane > c;
            if (side && ((dmask >> c) & 1u)) acc = pem_fma(-dv[c], xc, acc);
        }
    }
    if (out_lane) x[o] = acc;
}

// order[lvl[v] .. lvl[v + 1]): the tile rows of level v.  The workgroup runs the levels [lv0, lv1) in order, wave w of the grid
// taking the w-th tile row of each; with more than one level the grid is one workgroup, so what a level reads of an earlier one
// was written by this workgroup before the barrier.
template <typename VT, bool UPPER, int WAVES>
__global__ void __launch_bounds__(64 * WAVES) trsv_kernel(const int4 *__restrict__ rows, const int *__restrict__ order, const int *__restrict__ lvl,
                                                          const int lv0, const int lv1, const int *__restrict__ poff, const int *__restrict__ pminor,
                                                          const uint8_t *__restrict__ rci, const uint32_t *__restrict__ tile_rec,
                                                          const VT *__restrict__ vals, const VT *b, VT *x, const long long n, const int unit)
{
    __shared__ VT s_t[WAVES * 64];     // [wave][slot]: a
    __shared__ VT s_x[WAVES * 64];     // [wave][slot]: x
    __shared__ VT s_d[WAVES * 256];    // [wave][16 c + r]: the diagonal tile
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long w = (long long)blockIdx.x * WAVES + wv;
    for (int v = lv0; v < lv1; ++v) {   // (workgroup-uniform)
        const int w0 = lvl[v], width = lvl[v + 1] - w0;
        if (w < width)   // (wave-uniform)
            trsv_tile_row<VT, UPPER>(order[w0 + w], lane, s_t + wv * 64, s_x + wv * 64, s_d + wv * 256, rows, poff, pminor, rci, tile_rec, vals, b, x,
                                     n, unit);
        if (v + 1 < lv1) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __syncthreads();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
    }
}

// the rows without a stored diagonal entry: their count, and n - (the first of them) as a maximum (both start from 0)
__global__ void trsv_diag_kernel(const int4 *__restrict__ rows, const uint32_t *__restrict__ tile_rec, const long long n,
                                 unsigned long long *__restrict__ count, unsigned long long *__restrict__ first)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int dt = rows[i >> 4].z;
    const unsigned r = (unsigned)(i & 15);
    if (dt >= 0 && ((tile_rec[16 * (size_t)dt + r] >> r) & 1u)) return;
    atomicAdd(count, 1ull);
    atomicMax(first, (unsigned long long)(n - i));
}

}  // namespace

// ------------------------------------------------------------------------------------------
// the schedule (once per tiling and triangle; also ilu0.hip's, tiled_internal.h)
// ------------------------------------------------------------------------------------------
pem_status pem::ensure_trsv(pem_ctx *ctx, const pem_tiled *A, int uplo)
{
    TrsvSched &S = A->trsv[uplo];
    if (S.ready) return PEM_OK;
    const int TR = A->tile_rows;
    const size_t nt = (size_t)A->ntiles;
    std::vector<int> rp((size_t)TR + 1, 0), ci(nt);
    PEM_HIP(hipMemcpyAsync(rp.data(), A->tile_rowptr.p, sizeof(int) * rp.size(), hipMemcpyDeviceToHost, ctx->stream));
    if (nt) PEM_HIP(hipMemcpyAsync(ci.data(), A->tile_colidx.p, sizeof(int) * nt, hipMemcpyDeviceToHost, ctx->stream));
    PEM_HIP(hipStreamSynchronize(ctx->stream));
    // per tile row: the positions of its off-diagonal tiles on the chosen side, its diagonal tile, its level
    std::vector<int> h((size_t)4 * TR);
    std::vector<int> level((size_t)TR, 1);
    int levels = 0;
    for (int k = 0; k < TR; ++k) {
        const int P = uplo == PEM_TRSV_UPPER ? TR - 1 - k : k;
        const int *lo = ci.data() + rp[P], *hi = ci.data() + rp[P + 1];
        const int cut = (int)(std::lower_bound(lo, hi, P) - ci.data());
        const bool diag = cut < rp[P + 1] && ci[cut] == P;
        const int a = uplo == PEM_TRSV_UPPER ? cut + (diag ? 1 : 0) : rp[P], e = uplo == PEM_TRSV_UPPER ? rp[P + 1] : cut;
        int lv = 0;
        for (int p = a; p < e; ++p) lv = std::max(lv, level[ci[p]]);
        level[P] = lv + 1;
        levels = std::max(levels, lv + 1);
        h[4 * (size_t)P] = a;
        h[4 * (size_t)P + 1] = e;
        h[4 * (size_t)P + 2] = diag ? cut : -1;
        h[4 * (size_t)P + 3] = lv + 1;
    }
    // the tile rows by level (ascending inside a level) and the level offsets
    S.h_lvl.assign((size_t)levels + 1, 0);
    for (int P = 0; P < TR; ++P) ++S.h_lvl[level[P]];
    for (int v = 0; v < levels; ++v) S.h_lvl[v + 1] += S.h_lvl[v];
    S.order_off = h.size();
    S.lvl_off = S.order_off + (size_t)TR;
    h.resize(S.lvl_off + S.h_lvl.size());
    {
        std::vector<int> next(S.h_lvl.begin(), S.h_lvl.end() - 1);
        for (int P = 0; P < TR; ++P) h[S.order_off + next[level[P] - 1]++] = P;
    }
    std::copy(S.h_lvl.begin(), S.h_lvl.end(), h.begin() + S.lvl_off);
    S.max_width = 0;
    for (int v = 0; v < levels; ++v) S.max_width = std::max<int64_t>(S.max_width, S.h_lvl[v + 1] - S.h_lvl[v]);
    PEM_TRY(S.buf.reserve(sizeof(int) * h.size()));
    PEM_HIP(hipMemcpyAsync(S.buf.p, h.data(), sizeof(int) * h.size(), hipMemcpyHostToDevice, ctx->stream));
    // the rows without a stored diagonal entry (the read-back also ends the upload before h goes)
    int64_t *sc = ctx->d_scalars + 16;
    PEM_HIP(hipMemsetAsync(sc, 0, 2 * sizeof(int64_t), ctx->stream));
    PEM_LAUNCH(ctx, trsv_diag_kernel, grid_for((size_t)A->rows, 256), 256, S.buf.as<int4>(), A->tile_rec.as<uint32_t>(), (long long)A->rows,
               reinterpret_cast<unsigned long long *>(sc), reinterpret_cast<unsigned long long *>(sc + 1));
    int64_t got[2] = {0, 0};
    PEM_TRY(read_scalars(ctx, sc, 2, got));
    PEM_TRY(launch_status(ctx));
    S.missing_diag = got[0];
    S.first_missing_row = got[0] ? (int64_t)A->rows - got[1] + 1 : 0;
    S.ready = true;
    return PEM_OK;
}

namespace {

int trsv_merge_width(const pem_ctx *ctx) { return ctx->dbg_trsv_split ? 0 : TRSV_MERGE; }

template <typename VT, bool UPPER>
pem_status trsv_launch(pem_ctx *ctx, const pem_tiled *A, int unit, const VT *b, VT *x)
{
    const TrsvSched &S = A->trsv[UPPER];
    static const char *const names[2][2][2] = {{{"trsv_kernel<float,lower,level>", "trsv_kernel<float,lower,merged>"},
                                                {"trsv_kernel<float,upper,level>", "trsv_kernel<float,upper,merged>"}},
                                               {{"trsv_kernel<double,lower,level>", "trsv_kernel<double,lower,merged>"},
                                                {"trsv_kernel<double,upper,level>", "trsv_kernel<double,upper,merged>"}}};
    const int4 *rows = S.buf.as<int4>();
    const int *order = S.buf.as<int>() + S.order_off, *lvl = S.buf.as<int>() + S.lvl_off;
    trsv_for_launches(S, trsv_merge_width(ctx), [&](int v, int e, bool merged) {
        const char *name = names[sizeof(VT) == 8][UPPER][merged];
        if (merged) {
            PEM_LAUNCH_NAMED(ctx, name, (trsv_kernel<VT, UPPER, TRSV_MERGE>), 1, 64 * TRSV_MERGE, rows, order, lvl, v, e, A->tile_nnz_ptr.as<int>(),
                             A->tile_colidx.as<int>(), A->rowcolidx.as<uint8_t>(), A->tile_rec.as<uint32_t>(), A->vals.as<VT>(), b, x,
                             (long long)A->rows, unit);
        } else {
            const size_t width = (size_t)(S.h_lvl[v + 1] - S.h_lvl[v]);
            PEM_LAUNCH_NAMED(ctx, name, (trsv_kernel<VT, UPPER, TRSV_WIDE>), grid_for(width, TRSV_WIDE), 64 * TRSV_WIDE, rows, order, lvl, v, e,
                             A->tile_nnz_ptr.as<int>(), A->tile_colidx.as<int>(), A->rowcolidx.as<uint8_t>(), A->tile_rec.as<uint32_t>(),
                             A->vals.as<VT>(), b, x, (long long)A->rows, unit);
        }
    });
    return PEM_OK;
}

pem_status trsv_checks(pem_ctx *ctx, const pem_tiled *A, int uplo, const char *fn)
{
    if (!ctx || !A) {
        set_error("%s: null context or tiling", fn);
        return PEM_E_INVALID;
    }
    if (A->rows != A->cols) {
        set_error("%s: the tiling is %d x %d; a triangular solve needs a square one", fn, A->rows, A->cols);
        return PEM_E_INVALID;
    }
    if (uplo != PEM_TRSV_LOWER && uplo != PEM_TRSV_UPPER) {
        set_error("%s: unknown uplo %d (PEM_TRSV_LOWER = 0, PEM_TRSV_UPPER = 1)", fn, uplo);
        return PEM_E_INVALID;
    }
    return PEM_OK;
}

pem_status trsv_common(pem_ctx *ctx, const pem_tiled *A, int uplo, int unit_diag, const void *db, void *dx, int value_bytes, const char *fn)
{
    PEM_TRY(trsv_checks(ctx, A, uplo, fn));
    if (unit_diag != 0 && unit_diag != 1) {
        set_error("%s: unit_diag must be 0 or 1 (got %d)", fn, unit_diag);
        return PEM_E_INVALID;
    }
    if (A->value_bytes != value_bytes) {
        set_error("%s: the tiling holds %s values; use the %s entry point", fn, A->value_bytes == 4 ? "fp32" : "fp64",
                  A->value_bytes == 4 ? "_f32" : "fp64");
        return PEM_E_INVALID;
    }
    const size_t n = (size_t)A->rows;
    if (n == 0) return PEM_OK;
    if (!db || !dx) {
        set_error("%s: null vector", fn);
        return PEM_E_INVALID;
    }
    if (db != dx && Span(db, n * value_bytes).meets(Span(dx, n * value_bytes))) {
        set_error("%s: b and x overlap without being the same vector", fn);
        return PEM_E_INVALID;
    }
    PEM_ENTER(ctx);
    PEM_TRY(ensure_trsv(ctx, A, uplo));
    const TrsvSched &S = A->trsv[uplo];
    if (!unit_diag && S.missing_diag) {
        set_error("%s: row %lld has no stored diagonal entry (%lld such rows); store it or pass unit_diag = 1", fn,
                  (long long)S.first_missing_row, (long long)S.missing_diag);
        return PEM_E_INVALID;
    }
    if (value_bytes == 4)
        return uplo ? trsv_launch<float, true>(ctx, A, unit_diag, (const float *)db, (float *)dx)
                    : trsv_launch<float, false>(ctx, A, unit_diag, (const float *)db, (float *)dx);
    return uplo ? trsv_launch<double, true>(ctx, A, unit_diag, (const double *)db, (double *)dx)
                : trsv_launch<double, false>(ctx, A, unit_diag, (const double *)db, (double *)dx);
}

}  // namespace

extern "C" pem_status pem_tiled_trsv(pem_ctx *ctx, const pem_tiled *A, int uplo, int unit_diag, const double *db, double *dx)
{
    return trsv_common(ctx, A, uplo, unit_diag, db, dx, 8, "pem_tiled_trsv");
}

extern "C" pem_status pem_tiled_trsv_f32(pem_ctx *ctx, const pem_tiled *A, int uplo, int unit_diag, const float *db, float *dx)
{
    return trsv_common(ctx, A, uplo, unit_diag, db, dx, 4, "pem_tiled_trsv_f32");
}

extern "C" pem_status pem_tiled_trsv_info(pem_ctx *ctx, const pem_tiled *A, int uplo, pem_trsv_info *out)
{
    PEM_TRY(trsv_checks(ctx, A, uplo, "pem_tiled_trsv_info"));
    if (!out) {
        set_error("pem_tiled_trsv_info: null out");
        return PEM_E_INVALID;
    }
    *out = pem_trsv_info{};
    out->merge_width = trsv_merge_width(ctx);
    if (A->rows == 0) return PEM_OK;
    PEM_ENTER(ctx);
    PEM_TRY(ensure_trsv(ctx, A, uplo));
    const TrsvSched &S = A->trsv[uplo];
    out->levels = (int64_t)S.h_lvl.size() - 1;
    out->launches = trsv_for_launches(S, trsv_merge_width(ctx), [](int, int, bool) {});
    out->max_width = S.max_width;
    out->missing_diag = S.missing_diag;
    out->first_missing_row = S.first_missing_row;
    return PEM_OK;
}

extern "C" pem_status pem_test_trsv_split(pem_ctx *ctx, int on)
{
    if (!ctx || (on != 0 && on != 1)) {
        set_error("pem_test_trsv_split: null context, or on not 0 or 1");
        return PEM_E_INVALID;
    }
    ctx->dbg_trsv_split = on;
    return PEM_OK;
}
