// spmm.hip -- a tiling times a dense row-major block of vectors under a semiring (include/pem_spgemm.h, pem_tiled_spmm):
// Y = A (+).(x) X, or Y = A^T (+).(x) X, X nx x k and Y ny x k.  Column c of Y is bit for bit pem_tiled_mxv of column c of X.
//
// The walk is mxv's (mxv.hip): one wave per LINE (a tile row for A.X, a tile column for A^T.X), the line's entries loaded 64 at a
// time, one per lane, the lane's tile found by a shuffle search, (major, minor) decoded from the entry's (r << 4) | c byte, the chunk
// regrouped by major with 16 ballots and staged in the wave's LDS.  What is staged differs: the entry's value a and its X row index
// 16 * tile minor + minor, not x -- the x of an entry depends on the column.
// The fold maps lanes to (major, column): lane = g * W + w folds column cb * W + w (cb = the column block, the grid's second
// dimension) for the majors j * G + g, j = 0 .. 16 / G - 1, G = 64 / W groups side by side.  Adjacent lanes take adjacent columns,
// so an entry's X row is one coalesced W * value_bytes segment.  Every (major, column) is one serial chain in staged order, with
// mxv's very steps (MxOp, mx_internal.h): acc = step(acc, term(a, x), x).  Before the chains, the whole wave gathers the chunk's X
// rows into LDS (W loads in flight per lane), as mxv gathers x one entry per lane: a chain then reads only LDS, so a heavy row costs
// one gather latency per chunk, not one per few entries.  k = 1 with unit strides is mxv's own kernel.
// A column block re-walks A's line: about 9 B of A per entry against 8 * W B of X.  No atomics: every Y element is written once,
// by the lane that folded it; columns at or past k are never touched.
#include "spgemm_internal.h"
#include "tiled_internal.h"
#include "mx_internal.h"
#include <climits>

using namespace pem;

// lptr[L .. L+1]: the line's tile positions; poff[p]: entry offset of position p in walk order (poff[p1] closes the line);
// pbase[p] (COL only): the tile's first slot in vals / rci; pminor[p]: the tile index along X's rows; rci: (major << 4) | minor per
// slot.  X is nx x k with row stride ldx, Y nout x k with row stride ldy; this launch's column blocks start at cb0.
template <typename VT, int K, bool COL, int W>
__global__ void __launch_bounds__(256) spmm_kernel(const int *__restrict__ lptr, long long nlines, const int *__restrict__ poff,
                                                   const int *__restrict__ pbase, const int *__restrict__ pminor, const uint8_t *__restrict__ rci,
                                                   const VT *__restrict__ vals, const VT *__restrict__ X, long long ldx, VT *__restrict__ Y,
                                                   long long ldy, long long nout, long long k, long long cb0, int accumulate)
{
    using Op = MxOp<K>;
    constexpr int G = 64 / W;     // majors folded side by side
    constexpr int MPL = 16 / G;   // majors per lane
    __shared__ VT s_a[Op::reads_vals ? 4 * 64 : 1];    // [wave][slot]: the entry's value
    __shared__ int s_xr[Op::reads_x ? 4 * 64 : 1];     // [wave][slot]: the entry's X row
    __shared__ VT s_x[Op::reads_x ? 4 * 64 * W : 1];   // [wave][slot][w]: X at the entry's row, column cb * W + w
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long L = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (L >= nlines) return;   // (wave-uniform)
    VT *const my_a = s_a + (Op::reads_vals ? wv * 64 : 0);
    int *const my_xr = s_xr + (Op::reads_x ? wv * 64 : 0);
    VT *const my_x = s_x + (Op::reads_x ? wv * 64 * W : 0);
    const int g = lane / W, w = lane % W;
    const long long c = (cb0 + blockIdx.y) * W + w;
    const bool col_ok = c < k;
    VT acc[MPL];
#pragma unroll
    for (int j = 0; j < MPL; ++j) {
        acc[j] = Op::template start<VT>();
        const long long o = 16 * L + j * G + g;
        if (col_ok && accumulate && o < nout) acc[j] = Op::template from_y<VT>(Y[o * ldy + c]);
    }
    unsigned touched = 0;   // bit j: major j * G + g has an entry
    const int p0 = lptr[L], p1 = lptr[L + 1];
    if (p0 < p1) {
        const int e_end = poff[p1];
        int pc = p0;   // the tile holding the chunk's first entry (wave-uniform)
        for (int eb = poff[p0]; eb < e_end; eb += 64) {   // wave-uniform trip count
            const int mp = pc + lane;
            const bool lv = mp < p1;
            const int my_off = lv ? poff[mp] : INT_MAX;
            const int my_minor = lv ? pminor[mp] : 0;
            int my_base = 0;
            if constexpr (COL) my_base = lv ? pbase[mp] : 0;
            const int e = eb + lane;
            const int ti = chunk_tile_of(my_off, e);
            const int t_off = __shfl(my_off, ti, 64), t_minor = __shfl(my_minor, ti, 64);
            int t_base = 0;
            if constexpr (COL) t_base = __shfl(my_base, ti, 64);
            const int ti_last = __shfl(ti, 63, 64);
            int major = 16, xr = 0;
            VT a = VT(0);
            if (e < e_end) {
                const int slot = COL ? t_base + (e - t_off) : e;
                const unsigned rc = rci[slot];
                major = (int)(rc >> 4);
                if constexpr (Op::reads_vals) a = vals[slot];
                xr = 16 * t_minor + (int)(rc & 15u);
            }
            // regroup the chunk by major (mxv's ranking); the lane keeps the run (first slot, count) of each of its majors
            int slot = 0, run = 0;
            int first[MPL], cnt[MPL];
#pragma unroll
            for (int m = 0; m < 16; ++m) {
                const unsigned long long b = __ballot(major == m);
                const int n = __popcll(b);
                if (major == m) slot = run + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
                if (m % G == g) {
                    first[m / G] = run;
                    cnt[m / G] = n;
                }
                run += n;
            }
            wave_lds_sync();   // the previous chunk's folds have read the staging area
            if (major < 16) {
                if constexpr (Op::reads_vals) my_a[slot] = a;
                if constexpr (Op::reads_x) my_xr[slot] = xr;
            }
            wave_lds_sync();
            if constexpr (Op::reads_x) {   // the whole wave gathers the chunk's X rows (slots g, g + G, ...; W loads in flight per lane)
                const int nchunk = run;
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    const int s = g + i * G;
                    VT v = VT(0);
                    if (s < nchunk && col_ok) v = X[(long long)my_xr[s] * ldx + c];
                    my_x[s * W + w] = v;
                }
                wave_lds_sync();
            }
#pragma unroll
            for (int j = 0; j < MPL; ++j) {   // (lanes past column k fold zeros: their accumulators are never stored)
                const int f = first[j], n = cnt[j];
                if (n) touched |= 1u << j;
                VT r = acc[j];
                for (int q = 0; q < n; q += 4) {   // four LDS reads ahead of the chain
                    VT t4[4], x4[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const bool live = q + i < n;
                        t4[i] = VT(0);
                        x4[i] = VT(0);
                        if constexpr (Op::reads_vals)
                            if (live) t4[i] = my_a[f + q + i];
                        if constexpr (Op::reads_x)
                            if (live) x4[i] = my_x[(f + q + i) * W + w];
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const VT nr = Op::template step<VT>(r, Op::template term<VT>(t4[i], x4[i]), x4[i]);
                        r = q + i < n ? nr : r;
                    }
                }
                acc[j] = r;
            }
            // the next chunk starts in the tile of entry eb + 63, or in the one after it
            int pn = pc + ti_last;
            if (eb + 64 < e_end && pn + 1 < p1 && poff[pn + 1] <= eb + 64) ++pn;
            pc = pn;
        }
    }
    if (!col_ok) return;
#pragma unroll
    for (int j = 0; j < MPL; ++j) {
        const long long o = 16 * L + j * G + g;
        if (o < nout && (((touched >> j) & 1u) || !accumulate)) Y[o * ldy + c] = acc[j];
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
enum { SP_WIDTHS = 3 };
static constexpr int kSpWidth[SP_WIDTHS] = {4, 8, 16};

#define SP_NAMES_O(vt, s, o) {"spmm_kernel<" vt "," s "," o ",4>", "spmm_kernel<" vt "," s "," o ",8>", "spmm_kernel<" vt "," s "," o ",16>"}
#define SP_NAMES(vt, s) {SP_NAMES_O(vt, s, "rows"), SP_NAMES_O(vt, s, "cols")}
#define SP_NAMES_VT(vt)                                                                                                           \
    {SP_NAMES(vt, "plus_times"), SP_NAMES(vt, "min_plus"), SP_NAMES(vt, "max_plus"), SP_NAMES(vt, "max_times"),                  \
     SP_NAMES(vt, "plus_pair"), SP_NAMES(vt, "lor_land")}
static const char *const kSpNames[2][6][2][SP_WIDTHS] = {SP_NAMES_VT("float"), SP_NAMES_VT("double")};

// the width for k columns: the narrowest of 4, 8, 16 that holds them, 16 (and column blocks) past that.  The chunk's X rows take
// 64 * W values of LDS per wave, so W = 16 keeps four fp64 blocks of 256 on a CU.
static int sp_width_index(int64_t k) { return k <= 4 ? 0 : k <= 8 ? 1 : 2; }

template <typename VT, int K, int WI>
static pem_status sp_launch(pem_ctx *ctx, const pem_tiled *A, bool col, int64_t k, const VT *X, int64_t ldx, VT *Y, int64_t ldy,
                            int accumulate)
{
    constexpr int W = kSpWidth[WI];
    const char *name = kSpNames[sizeof(VT) == 8][K][col][WI];
    const long long nlines = col ? A->tile_cols : A->tile_rows;
    const int64_t nblocks = k / W + (k % W != 0);
    const unsigned gx = grid_for((size_t)nlines * 64, 256);
    for (int64_t cb0 = 0; cb0 < nblocks; cb0 += 65535) {   // (the grid's second dimension holds at most 65535 column blocks)
        const dim3 grid(gx, (unsigned)std::min<int64_t>(65535, nblocks - cb0));
        if (col)
            PEM_LAUNCH_NAMED(ctx, name, (spmm_kernel<VT, K, true, W>), grid, 256, A->tile_colptr.as<int>(), nlines, A->mx_csc_off.as<int>(),
                             A->mx_csc_base.as<int>(), A->tile_rowidx.as<int>(), A->mx_rci_t.as<uint8_t>(), A->vals_t.as<VT>(), X,
                             (long long)ldx, Y, (long long)ldy, (long long)A->cols, (long long)k, (long long)cb0, accumulate);
        else
            PEM_LAUNCH_NAMED(ctx, name, (spmm_kernel<VT, K, false, W>), grid, 256, A->tile_rowptr.as<int>(), nlines,
                             A->tile_nnz_ptr.as<int>(), (const int *)nullptr, A->tile_colidx.as<int>(), A->rowcolidx.as<uint8_t>(),
                             A->vals.as<VT>(), X, (long long)ldx, Y, (long long)ldy, (long long)A->rows, (long long)k, (long long)cb0,
                             accumulate);
    }
    return PEM_OK;
}

template <typename VT, int K>
static pem_status sp_width(pem_ctx *ctx, const pem_tiled *A, bool col, int64_t k, const VT *X, int64_t ldx, VT *Y, int64_t ldy,
                           int accumulate)
{
    switch (sp_width_index(k)) {
    case 0: return sp_launch<VT, K, 0>(ctx, A, col, k, X, ldx, Y, ldy, accumulate);
    case 1: return sp_launch<VT, K, 1>(ctx, A, col, k, X, ldx, Y, ldy, accumulate);
    default: return sp_launch<VT, K, 2>(ctx, A, col, k, X, ldx, Y, ldy, accumulate);
    }
}

template <typename VT>
static pem_status sp_run(pem_ctx *ctx, const pem_tiled *A, int semiring, bool col, int64_t k, const VT *X, int64_t ldx, VT *Y, int64_t ldy,
                         int accumulate)
{
    if (k == 0 || (col ? A->tile_cols : A->tile_rows) == 0) return PEM_OK;   // no output
    if (col) PEM_TRY(ensure_mx_cols(ctx, A));
    if (k == 1 && ldx == 1 && ldy == 1) return mxv_semiring(ctx, A, semiring, col, X, Y, accumulate);   // one contiguous vector: mxv
    switch (semiring) {
    case 0: return sp_width<VT, 0>(ctx, A, col, k, X, ldx, Y, ldy, accumulate);
    case 1: return sp_width<VT, 1>(ctx, A, col, k, X, ldx, Y, ldy, accumulate);
    case 2: return sp_width<VT, 2>(ctx, A, col, k, X, ldx, Y, ldy, accumulate);
    case 3: return sp_width<VT, 3>(ctx, A, col, k, X, ldx, Y, ldy, accumulate);
    case 4: return sp_width<VT, 4>(ctx, A, col, k, X, ldx, Y, ldy, accumulate);
    default: return sp_width<VT, 5>(ctx, A, col, k, X, ldx, Y, ldy, accumulate);
    }
}

static bool sp_flag_ok(int v) { return v == 0 || v == 1; }

static pem_status spmm_common(pem_ctx *ctx, const pem_tiled *A, int semiring, int transpose, int64_t k, const void *dX, int64_t ldx,
                              void *dY, int64_t ldy, int accumulate, int value_bytes, const char *fn)
{
    if (!ctx || !A) {
        set_error("%s: null context or tiling", fn);
        return PEM_E_INVALID;
    }
    if (semiring < PEM_SEMIRING_PLUS_TIMES || semiring > PEM_SEMIRING_LOR_LAND) {
        set_error("%s: unknown semiring %d (PEM_SEMIRING_PLUS_TIMES .. PEM_SEMIRING_LOR_LAND = 0 .. 5)", fn, semiring);
        return PEM_E_INVALID;
    }
    if (!sp_flag_ok(transpose) || !sp_flag_ok(accumulate)) {
        set_error("%s: transpose and accumulate must be 0 or 1 (got %d, %d)", fn, transpose, accumulate);
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
    if (A->value_bytes != value_bytes) {
        set_error("%s: the tiling holds %s values; use the %s entry point", fn, A->value_bytes == 4 ? "fp32" : "fp64",
                  A->value_bytes == 4 ? "_f32" : "fp64");
        return PEM_E_INVALID;
    }
    const bool col = transpose == 1;
    const int64_t nx = col ? A->rows : A->cols, ny = col ? A->cols : A->rows;
    if ((nx > 0 && k > 0 && !dX) || (ny > 0 && k > 0 && !dY)) {
        set_error("%s: null X or Y", fn);
        return PEM_E_INVALID;
    }
    unsigned __int128 xlo, xhi, ylo, yhi;
    if (!sp_span(dX, nx, k, ldx, value_bytes, &xlo, &xhi) || !sp_span(dY, ny, k, ldy, value_bytes, &ylo, &yhi)) {
        set_error("%s: rows x row stride overflows int64 (X %lld x %lld, Y %lld x %lld)", fn, (long long)nx, (long long)ldx, (long long)ny,
                  (long long)ldy);
        return PEM_E_INVALID;
    }
    if (xlo < xhi && ylo < yhi && xlo < yhi && ylo < xhi) {
        set_error("%s: X and Y overlap", fn);
        return PEM_E_INVALID;
    }
    PEM_ENTER(ctx);
    if (value_bytes == 4) return sp_run<float>(ctx, A, semiring, col, k, (const float *)dX, ldx, (float *)dY, ldy, accumulate);
    return sp_run<double>(ctx, A, semiring, col, k, (const double *)dX, ldx, (double *)dY, ldy, accumulate);
}

extern "C" pem_status pem_tiled_spmm(pem_ctx *ctx, const pem_tiled *A, int semiring, int transpose, int64_t k, const double *dX, int64_t ldx,
                                     double *dY, int64_t ldy, int accumulate)
{
    return spmm_common(ctx, A, semiring, transpose, k, dX, ldx, dY, ldy, accumulate, 8, "pem_tiled_spmm");
}

extern "C" pem_status pem_tiled_spmm_f32(pem_ctx *ctx, const pem_tiled *A, int semiring, int transpose, int64_t k, const float *dX,
                                         int64_t ldx, float *dY, int64_t ldy, int accumulate)
{
    return spmm_common(ctx, A, semiring, transpose, k, dX, ldx, dY, ldy, accumulate, 4, "pem_tiled_spmm_f32");
}
