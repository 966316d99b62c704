// sddmm.hip -- the sampled dense-dense product (include/pem_spgemm.h, pem_tiled_sddmm / pem_tiled_set_values_sddmm): the values
// of a tiling become R(i, j) = (+)_c X[i, c] (x) Y[j, c] at the tiling's own stored positions, X rows x k and Y cols x k dense
// row-major device blocks.  The pattern is never touched and the old values are read only under accumulate.
//
// The walk is spmm's row walk (spmm.hip): one wave per tile row, the line's entries loaded 64 at a time, one per lane, the lane's
// tile found by a shuffle search, (r, c) decoded from the entry's (r << 4) | c byte.  No regrouping: the lane keeps its entry and
// folds its whole chain, acc = step(acc, term(X[i, c], Y[j, c]), Y[j, c]) in ascending c with mxv's very steps (MxOp,
// mx_internal.h), so plus_times is the fma chain from 0 (or from the old value).
// k is processed in column chunks of W (4, 8 or 16: the narrowest that holds k, 16 past that).  Per chunk the wave stages in its
// own LDS the tile row's 16 X rows once (16 x W) and every entry's Y row segment (64 x W), both with lanes along the columns, so
// a row segment is one coalesced W * value_bytes read; the chains then read only LDS, and while they run on one chunk the loads
// of the next are in flight (registers, written to LDS at the top of the next trip).  Staged rows have a pitch of W + 1 values:
// lanes read different rows at a common column, and an odd pitch spreads them over the banks (X rows shared by several lanes
// broadcast).  What is NOT done: a tile's entries that share a column stage the same Y row once each -- the staging is per
// entry, as a gather is, and relies on the cache for the reuse inside a tile ("Sampled dense-dense product").
// The lane writes its value to vals and, through vmap_t (values.hip), to vals_t: every value once, no atomics.
#include "spgemm_internal.h"
#include "tiled_internal.h"
#include "mx_internal.h"
#include <climits>

using namespace pem;

// lptr[L .. L+1]: the tile row's tiles; poff[p]: first entry of tile p (poff[p1] closes the line); pminor[p]: tile column; rci:
// (r << 4) | c per entry.  X is rows x k with row stride ldx, Y (the tiling's cols) x k with row stride ldy.  vals_t null: only
// vals is written (the builder derives vals_t afterwards).
template <typename VT, int K, int W>
__global__ void __launch_bounds__(256) sddmm_kernel(const int *__restrict__ lptr, long long nlines, const int *__restrict__ poff,
                                                    const int *__restrict__ pminor, const uint8_t *__restrict__ rci, const VT *__restrict__ X,
                                                    long long ldx, const VT *__restrict__ Y, long long ldy, long long rows, long long k,
                                                    int accumulate, VT *__restrict__ vals, const int *__restrict__ vmap_t,
                                                    VT *__restrict__ vals_t)
{
    using Op = MxOp<K>;
    constexpr int G = 64 / W;    // staged rows loaded side by side
    constexpr int P = W + 1;     // pitch of a staged row
    __shared__ VT s_x[Op::reads_x ? 4 * 16 * P : 1];   // [wave][local row][column of the chunk]
    __shared__ VT s_y[Op::reads_x ? 4 * 64 * P : 1];   // [wave][lane's entry][column of the chunk]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long L = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (L >= nlines) return;   // (wave-uniform)
    VT *const my_x = s_x + (Op::reads_x ? wv * 16 * P : 0);
    VT *const my_y = s_y + (Op::reads_x ? wv * 64 * P : 0);
    const int g = lane / W, w = lane % W;
    const int p0 = lptr[L], p1 = lptr[L + 1];
    if (p0 >= p1) return;
    const long long nblocks = k / W + (k % W != 0);
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
        const bool live = e < e_end;
        int r = 0, yr = -1;   // the entry's local row and its row of Y (-1: no entry)
        VT acc = Op::template start<VT>();
        if (live) {
            const unsigned rc = rci[e];
            r = (int)(rc >> 4);
            yr = 16 * t_minor + (int)(rc & 15u);
            if (accumulate) acc = Op::template from_y<VT>(vals[e]);
        }
        // the chunk's operands, one column chunk ahead: registers filled by fetch(cb) go to LDS at the top of trip cb, and the
        // loads of chunk cb + 1 are in flight while the chains run on chunk cb
        long long xo[16 / G], yo[W];   // element offsets of the lane's staged rows at column w (-1: no row)
        VT px[16 / G], py[W];
        if constexpr (Op::reads_x) {
#pragma unroll
            for (int i = 0; i < 16 / G; ++i) {   // the tile row's X rows g, g + G, ...
                const long long xi = 16 * L + g + i * G;
                xo[i] = xi < rows ? xi * ldx + w : -1;
            }
#pragma unroll
            for (int i = 0; i < W; ++i) {   // the Y rows of the entries of lanes g, g + G, ...
                const int ys = __shfl(yr, g + i * G, 64);
                yo[i] = ys >= 0 ? (long long)ys * ldy + w : -1;
            }
        }
        auto fetch = [&](const long long cb) {
            const long long c0 = cb * W;
            const bool col_ok = c0 + w < k;
#pragma unroll
            for (int i = 0; i < 16 / G; ++i) px[i] = (col_ok && xo[i] >= 0) ? X[xo[i] + c0] : VT(0);
#pragma unroll
            for (int i = 0; i < W; ++i) py[i] = (col_ok && yo[i] >= 0) ? Y[yo[i] + c0] : VT(0);
        };
        if constexpr (Op::reads_x)
            if (nblocks > 0) fetch(0);
        for (long long cb = 0; cb < nblocks; ++cb) {
            const long long c0 = cb * W;
            const int kw = (int)(k - c0 < W ? k - c0 : W);   // live columns of this chunk (wave-uniform)
            if constexpr (Op::reads_x) {
                wave_lds_sync();   // the previous chunk's chains have read the staging area
#pragma unroll
                for (int i = 0; i < 16 / G; ++i) my_x[(g + i * G) * P + w] = px[i];
#pragma unroll
                for (int i = 0; i < W; ++i) my_y[(g + i * G) * P + w] = py[i];
                wave_lds_sync();
                if (cb + 1 < nblocks) fetch(cb + 1);
            }
#pragma unroll
            for (int q = 0; q < W; q += 4) {   // four LDS reads ahead of the chain
                VT x4[4], y4[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    x4[i] = VT(0);
                    y4[i] = VT(0);
                    if constexpr (Op::reads_x) {
                        x4[i] = my_x[r * P + q + i];
                        y4[i] = my_y[lane * P + q + i];
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {   // (columns at or past k fold nothing: a -0.0 accumulator must stay -0.0)
                    const VT nr = Op::template step<VT>(acc, Op::template term<VT>(x4[i], y4[i]), y4[i]);
                    acc = q + i < kw ? nr : acc;
                }
            }
        }
        if (live) {
            vals[e] = acc;
            if (vals_t) vals_t[vmap_t[e]] = acc;
        }
        // the next chunk starts in the tile of entry eb + 63, or in the one after it
        int pn = pc + ti_last;
        if (eb + 64 < e_end && pn + 1 < p1 && poff[pn + 1] <= eb + 64) ++pn;
        pc = pn;
    }
}

// the exclusive scan of the tile-head flags derive_tiled reads, straight from the tile offsets: entry e of tile t has t heads in
// front of it if it is the tile's first entry, else t + 1; headx[nnz] = ntiles.  16 lanes per tile.
__global__ void __launch_bounds__(256) sddmm_headx_kernel(const int *__restrict__ tile_nnz_ptr, long long nt, int *__restrict__ headx)
{
    const long long t = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int r = threadIdx.x & 15;
    if (t >= nt) return;
    const int e0 = tile_nnz_ptr[t], e1 = tile_nnz_ptr[t + 1];
    for (int e = e0 + r; e < e1; e += 16) headx[e] = e == e0 ? (int)t : (int)t + 1;
    if (t == nt - 1 && r == 0) headx[e1] = (int)nt;
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
void pem::tile_headx(pem_ctx *ctx, const pem_tiled *S, int *headx)
{
    PEM_LAUNCH(ctx, sddmm_headx_kernel, grid_for(16 * (size_t)S->ntiles, 256), 256, S->tile_nnz_ptr.as<int>(), (long long)S->ntiles, headx);
}

enum { SD_WIDTHS = 3 };
static constexpr int kSdWidth[SD_WIDTHS] = {4, 8, 16};

#define SD_NAMES(vt, s) {"sddmm_kernel<" vt "," s ",4>", "sddmm_kernel<" vt "," s ",8>", "sddmm_kernel<" vt "," s ",16>"}
#define SD_NAMES_VT(vt) \
    {SD_NAMES(vt, "plus_times"), SD_NAMES(vt, "min_plus"), SD_NAMES(vt, "max_plus"), SD_NAMES(vt, "max_times"), SD_NAMES(vt, "plus_pair"), \
     SD_NAMES(vt, "lor_land")}
static const char *const kSdNames[2][6][SD_WIDTHS] = {SD_NAMES_VT("float"), SD_NAMES_VT("double")};

// the chunk width for k columns: the narrowest of 4, 8, 16 that holds them, 16 (and several chunks) past that.  W = 16 stages
// 80 rows of 17 values per wave: 42.5 KB of LDS per fp64 block of 256, three blocks on a CU.
static int sd_width_index(int64_t k) { return k <= 4 ? 0 : k <= 8 ? 1 : 2; }

// S gives the structure (row walk), the values go to vals and (unless null) through vmap_t to vals_t
template <typename VT, int K, int WI>
static void sd_launch(pem_ctx *ctx, const pem_tiled *S, int64_t k, const VT *X, int64_t ldx, const VT *Y, int64_t ldy, int accumulate, VT *vals,
                      const int *vmap_t, VT *vals_t)
{
    constexpr int W = kSdWidth[WI];
    const long long nlines = S->tile_rows;
    PEM_LAUNCH_NAMED(ctx, kSdNames[sizeof(VT) == 8][K][WI], (sddmm_kernel<VT, K, W>), grid_for((size_t)nlines * 64, 256), 256,
                     S->tile_rowptr.as<int>(), nlines, S->tile_nnz_ptr.as<int>(), S->tile_colidx.as<int>(), S->rowcolidx.as<uint8_t>(), X,
                     (long long)ldx, Y, (long long)ldy, (long long)S->rows, (long long)k, accumulate, vals, vmap_t, vals_t);
}

template <typename VT, int K>
static void sd_width(pem_ctx *ctx, const pem_tiled *S, int64_t k, const VT *X, int64_t ldx, const VT *Y, int64_t ldy, int accumulate, VT *vals,
                     const int *vmap_t, VT *vals_t)
{
    switch (sd_width_index(k)) {
    case 0: return sd_launch<VT, K, 0>(ctx, S, k, X, ldx, Y, ldy, accumulate, vals, vmap_t, vals_t);
    case 1: return sd_launch<VT, K, 1>(ctx, S, k, X, ldx, Y, ldy, accumulate, vals, vmap_t, vals_t);
    default: return sd_launch<VT, K, 2>(ctx, S, k, X, ldx, Y, ldy, accumulate, vals, vmap_t, vals_t);
    }
}

template <typename VT>
static void sd_run(pem_ctx *ctx, const pem_tiled *S, int semiring, int64_t k, const void *dX, int64_t ldx, const void *dY, int64_t ldy,
                   int accumulate, void *vals, const int *vmap_t, void *vals_t)
{
    const VT *X = static_cast<const VT *>(dX), *Y = static_cast<const VT *>(dY);
    VT *v = static_cast<VT *>(vals), *vt = static_cast<VT *>(vals_t);
    switch (semiring) {
    case 0: return sd_width<VT, 0>(ctx, S, k, X, ldx, Y, ldy, accumulate, v, vmap_t, vt);
    case 1: return sd_width<VT, 1>(ctx, S, k, X, ldx, Y, ldy, accumulate, v, vmap_t, vt);
    case 2: return sd_width<VT, 2>(ctx, S, k, X, ldx, Y, ldy, accumulate, v, vmap_t, vt);
    case 3: return sd_width<VT, 3>(ctx, S, k, X, ldx, Y, ldy, accumulate, v, vmap_t, vt);
    case 4: return sd_width<VT, 4>(ctx, S, k, X, ldx, Y, ldy, accumulate, v, vmap_t, vt);
    default: return sd_width<VT, 5>(ctx, S, k, X, ldx, Y, ldy, accumulate, v, vmap_t, vt);
    }
}

// the checks all four entry points share (the handles are not null); nothing here touches the device
static pem_status sd_check(const pem_tiled *S, int semiring, int64_t k, const void *dX, int64_t ldx, const void *dY, int64_t ldy,
                           int value_bytes, const char *fn)
{
    if (semiring < PEM_SEMIRING_PLUS_TIMES || semiring > PEM_SEMIRING_LOR_LAND) {
        set_error("%s: unknown semiring %d (PEM_SEMIRING_PLUS_TIMES .. PEM_SEMIRING_LOR_LAND = 0 .. 5)", fn, semiring);
        return PEM_E_INVALID;
    }
    if (k < 0) {
        set_error("%s: k = %lld columns is negative", fn, (long long)k);
        return PEM_E_INVALID;
    }
    const int64_t kmin = k > 1 ? k : 1;
    if (ldx < kmin || ldy < kmin) {
        set_error("%s: the row strides must be at least max(k, 1) = %lld (ldx = %lld, ldy = %lld)", fn, (long long)kmin, (long long)ldx,
                  (long long)ldy);
        return PEM_E_INVALID;
    }
    const bool reads = semiring != PEM_SEMIRING_PLUS_PAIR;
    if (reads && k > 0 && ((S->rows > 0 && !dX) || (S->cols > 0 && !dY))) {
        set_error("%s: null X or Y", fn);
        return PEM_E_INVALID;
    }
    unsigned __int128 lo, hi;
    if (!sp_span(dX, S->rows, k, ldx, value_bytes, &lo, &hi) || !sp_span(dY, S->cols, k, ldy, value_bytes, &lo, &hi)) {
        set_error("%s: rows x row stride overflows int64 (X %lld x %lld, Y %lld x %lld)", fn, (long long)S->rows, (long long)ldx,
                  (long long)S->cols, (long long)ldy);
        return PEM_E_INVALID;
    }
    return PEM_OK;
}

static pem_status sddmm_in_place(pem_ctx *ctx, pem_tiled *t, int semiring, int64_t k, const void *dX, int64_t ldx, const void *dY, int64_t ldy,
                                 int accumulate, int value_bytes, const char *fn)
{
    if (!ctx || !t) {
        set_error("%s: null context or tiling", fn);
        return PEM_E_INVALID;
    }
    if (accumulate != 0 && accumulate != 1) {
        set_error("%s: accumulate must be 0 or 1 (got %d)", fn, accumulate);
        return PEM_E_INVALID;
    }
    PEM_TRY(sd_check(t, semiring, k, dX, ldx, dY, ldy, value_bytes, fn));
    if (t->value_bytes != value_bytes) {
        set_error("%s: the tiling holds %s values; use the %s entry point", fn, t->value_bytes == 4 ? "fp32" : "fp64",
                  t->value_bytes == 4 ? "_f32" : "fp64");
        return PEM_E_INVALID;
    }
    if (t->nnz) {
        PEM_ENTER(ctx);
        PEM_TRY(ensure_vmap_t(ctx, t));
        if (value_bytes == 4)
            sd_run<float>(ctx, t, semiring, k, dX, ldx, dY, ldy, accumulate, t->vals.p, t->vmap_t.as<int>(), t->vals_t.p);
        else
            sd_run<double>(ctx, t, semiring, k, dX, ldx, dY, ldy, accumulate, t->vals.p, t->vmap_t.as<int>(), t->vals_t.p);
    }
    ++t->value_version;
    return PEM_OK;
}

// S's sorted tile payload copied, the values computed on S's structure into T's vals, everything else derived
static pem_status sddmm_build(pem_ctx *ctx, const pem_tiled *S, int semiring, int64_t k, const void *dX, int64_t ldx, const void *dY,
                              int64_t ldy, int value_bytes, pem_tiled *T)
{
    hipStream_t st = ctx->stream;
    const size_t nnz = (size_t)S->nnz, nt = (size_t)S->ntiles;
    PEM_TRY(zero_flags(ctx));
    set_tiled_shape(T, value_bytes, S->rows, S->cols);
    T->nnz = S->nnz;
    T->ntiles = S->ntiles;
    const int bits_tr = bits_for((uint64_t)T->tile_rows), bits_tc = bits_for((uint64_t)T->tile_cols);
    PEM_TRY(reserve_payload(ctx, T));
    int *headx;
    PEM_TRY(begin_payload(ctx, T, &headx));
    if (nnz) {
        PEM_HIP(hipMemcpyAsync(T->tile_keys.p, S->tile_keys.p, sizeof(long long) * nt, hipMemcpyDeviceToDevice, st));
        PEM_HIP(hipMemcpyAsync(T->tile_nnz_ptr.p, S->tile_nnz_ptr.p, sizeof(int) * (nt + 1), hipMemcpyDeviceToDevice, st));
        PEM_HIP(hipMemcpyAsync(T->rowcolidx.p, S->rowcolidx.p, nnz, hipMemcpyDeviceToDevice, st));
        tile_headx(ctx, S, headx);
        if (value_bytes == 4)
            sd_run<float>(ctx, S, semiring, k, dX, ldx, dY, ldy, 0, T->vals.p, nullptr, nullptr);
        else
            sd_run<double>(ctx, S, semiring, k, dX, ldx, dY, ldy, 0, T->vals.p, nullptr, nullptr);
    }
    PEM_TRY(derive_tiled(ctx, T, headx, bits_tr, bits_tc));
    int hf[NUM_FLAGS];
    PEM_TRY(read_flags(ctx, hf));
    return check_internal(hf);
}

static pem_status sddmm_new(pem_ctx *ctx, const pem_tiled *S, int semiring, int64_t k, const void *dX, int64_t ldx, const void *dY, int64_t ldy,
                            pem_tiled **out, int value_bytes, const char *fn)
{
    if (!ctx || !S || !out) {
        set_error("%s: null context, tiling or output", fn);
        return PEM_E_INVALID;
    }
    *out = nullptr;
    PEM_TRY(sd_check(S, semiring, k, dX, ldx, dY, ldy, value_bytes, fn));
    return build_derived(ctx, out, [&](pem_tiled *T) { return sddmm_build(ctx, S, semiring, k, dX, ldx, dY, ldy, value_bytes, T); });
}

extern "C" pem_status pem_tiled_set_values_sddmm(pem_ctx *ctx, pem_tiled *t, int semiring, int64_t k, const double *dX, int64_t ldx,
                                                 const double *dY, int64_t ldy, int accumulate)
{
    return sddmm_in_place(ctx, t, semiring, k, dX, ldx, dY, ldy, accumulate, 8, "pem_tiled_set_values_sddmm");
}

extern "C" pem_status pem_tiled_set_values_sddmm_f32(pem_ctx *ctx, pem_tiled *t, int semiring, int64_t k, const float *dX, int64_t ldx,
                                                     const float *dY, int64_t ldy, int accumulate)
{
    return sddmm_in_place(ctx, t, semiring, k, dX, ldx, dY, ldy, accumulate, 4, "pem_tiled_set_values_sddmm_f32");
}

extern "C" pem_status pem_tiled_sddmm(pem_ctx *ctx, const pem_tiled *S, int semiring, int64_t k, const double *dX, int64_t ldx,
                                      const double *dY, int64_t ldy, pem_tiled **out)
{
    return sddmm_new(ctx, S, semiring, k, dX, ldx, dY, ldy, out, 8, "pem_tiled_sddmm");
}

extern "C" pem_status pem_tiled_sddmm_f32(pem_ctx *ctx, const pem_tiled *S, int semiring, int64_t k, const float *dX, int64_t ldx,
                                          const float *dY, int64_t ldy, pem_tiled **out)
{
    return sddmm_new(ctx, S, semiring, k, dX, ldx, dY, ldy, out, 4, "pem_tiled_sddmm_f32");
}
