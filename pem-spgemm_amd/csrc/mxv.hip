// mxv.hip -- sparse matrix x dense vector under a semiring, and row / column reductions, of any tiling (include/pem_spgemm.h,
// pem_tiled_mxv / pem_tiled_reduce): y = A (+).(x) x, y = A^T (+).(x) x, y_i = the (+)-fold of row i's (column j's) stored values.
//
// Every output is one serial chain over its line's entries in ascending index (the plan's order: A.X with X a column gives the same
// bits), so the only parallel work is the loads and the gathers.  One wave owns one LINE: a tile row (16 matrix rows) for A.x, a
// tile column (16 matrix columns) for A^T.x.  Its entries are walked in chunks of 64, one entry per lane:
//   decode     the lane's tile by a shuffle search over the offsets of the (at most 64) tiles the chunk touches, its (major, minor)
//              from the 1-byte (r << 4) | c of the entry (major: the output inside the line, minor: the x index inside the tile);
//              its value and, for mxv, x[16 * tile's minor index + minor].
//   rank       16 ballots (one per major) give every entry its slot in the chunk when the chunk is regrouped by major, the order
//              inside a major kept: the tiles ascend in the minor index and so do a tile's entries of one row (column).
//   stage      the lane writes its (a, x) pair -- or, for the semirings without an fma and for the reductions, the one term that
//              enters the fold -- into the wave's LDS at that slot.
//   chain      lane m (m < 16) folds the run of major m from LDS into its accumulator, four reads ahead of the arithmetic.
// A line of thousands of entries in one row is therefore loaded by the whole wave and chained by one lane with no global load on
// the chain: this is the long-row path, and it needs no binning -- a short line is one chunk.
// Row walk: the tiling's own tile_rowptr, tile_nnz_ptr, tile_colidx, rowcolidx and vals (entries of a tile row are contiguous).
// Column walk: the tiles of a tile column are not contiguous in vals_t, so the first column call builds a schedule kept with the
// tiling: per CSC position the entry offset in column-walk order (a scan of the tiles' counts) and the tile's first slot in vals_t,
// and per slot of vals_t the entry's (c << 4) | r.  Then tile_colptr, tile_rowidx and vals_t as they are.
// Reductions are the same kernel with the x gather compiled out (the kind K below).  No atomics: every value is written by the one
// lane that folded it.
#include "spgemm_internal.h"
#include "tiled_internal.h"
#include "mx_internal.h"
#include <climits>

using namespace pem;

// the folds (MxOp, mx_internal.h): K < 6 is a pem_semiring (mxv), K = 6 + op a pem_binop (reduce)

// ------------------------------------------------------------------------------------------
// the walk: one wave per line, one entry per lane (header comment)
// ------------------------------------------------------------------------------------------
// lptr[L .. L+1]: the line's tile positions; poff[p]: entry offset of position p in walk order (poff[p1] closes the line);
// pbase[p] (COL only): the tile's first slot in vals / rci; pminor[p]: the tile index along x (tile column for rows, tile row
// for columns); rci: (major << 4) | minor per slot; y has nout entries, 16 per line.
template <typename VT, int K, bool COL>
__global__ void __launch_bounds__(256) mxv_kernel(const int *__restrict__ lptr, long long nlines, const int *__restrict__ poff,
                                                  const int *__restrict__ pbase, const int *__restrict__ pminor, const uint8_t *__restrict__ rci,
                                                  const VT *__restrict__ vals, const VT *__restrict__ x, VT *__restrict__ y, long long nout,
                                                  int accumulate)
{
    using Op = MxOp<K>;
    __shared__ VT s_t[4 * 64];                    // [wave][slot]: a (plus_times) or the entry's term
    __shared__ VT s_x[Op::pair ? 4 * 64 : 1];     // [wave][slot]: x (plus_times)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long L = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (L >= nlines) return;   // (wave-uniform)
    VT *const my_t = s_t + wv * 64;
    VT *const my_x = s_x + (Op::pair ? wv * 64 : 0);
    const long long o = 16 * L + lane;
    const bool out_lane = lane < 16 && o < nout;
    VT acc = Op::template start<VT>();
    if (out_lane && accumulate) acc = Op::template from_y<VT>(y[o]);
    int touched = 0;
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
            int ti = 0;   // the last of the chunk's tiles starting at or before e (tiles hold 1..256 entries: at most 64 of them)
#pragma unroll
            for (int step = 32; step > 0; step >>= 1) {
                const int probe = __shfl(my_off, ti + step, 64);
                if (probe <= e) ti += step;
            }
            const int t_off = __shfl(my_off, ti, 64), t_minor = __shfl(my_minor, ti, 64);
            int t_base = 0;
            if constexpr (COL) t_base = __shfl(my_base, ti, 64);
            const int ti_last = __shfl(ti, 63, 64);
            int major = 16;
            VT a = VT(0), xv = VT(0);
            if (e < e_end) {
                const int slot = COL ? t_base + (e - t_off) : e;
                const unsigned rc = rci[slot];
                major = (int)(rc >> 4);
                if constexpr (Op::reads_vals) a = vals[slot];
                if constexpr (Op::reads_x) xv = x[16 * (size_t)t_minor + (rc & 15u)];
            }
            // regroup the chunk by major: slot = entries of smaller majors + entries of the same major in lower lanes
            int slot = 0, my_first = 0, my_cnt = 0, run = 0;
#pragma unroll
            for (int m = 0; m < 16; ++m) {
                const unsigned long long b = __ballot(major == m);
                const int n = __popcll(b);
                if (major == m) slot = run + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
                if (lane == m) {
                    my_first = run;
                    my_cnt = n;
                }
                run += n;
            }
            mx_wave_sync();   // the previous chunk's chain has read the staging area
            if (major < 16) {
                if constexpr (Op::pair) {
                    my_t[slot] = a;
                    my_x[slot] = xv;
                } else {
                    my_t[slot] = Op::template term<VT>(a, xv);
                }
            }
            mx_wave_sync();
            touched |= my_cnt;
            const VT *pt = my_t + my_first;
            const VT *px = my_x + (Op::pair ? my_first : 0);
            int k = 0;
            for (; k + 4 <= my_cnt; k += 4) {   // four reads ahead of the chain
                const VT t0 = pt[k], t1 = pt[k + 1], t2 = pt[k + 2], t3 = pt[k + 3];
                VT x0 = VT(0), x1 = VT(0), x2 = VT(0), x3 = VT(0);
                if constexpr (Op::pair) x0 = px[k], x1 = px[k + 1], x2 = px[k + 2], x3 = px[k + 3];
                acc = Op::template step<VT>(acc, t0, x0);
                acc = Op::template step<VT>(acc, t1, x1);
                acc = Op::template step<VT>(acc, t2, x2);
                acc = Op::template step<VT>(acc, t3, x3);
            }
            for (; k < my_cnt; ++k) acc = Op::template step<VT>(acc, pt[k], Op::pair ? px[k] : VT(0));
            // the next chunk starts in the tile of entry eb + 63, or in the one after it
            int pn = pc + ti_last;
            if (eb + 64 < e_end && pn + 1 < p1 && poff[pn + 1] <= eb + 64) ++pn;
            pc = pn;
        }
    }
    if (out_lane && (touched || !accumulate)) y[o] = acc;
}

// ------------------------------------------------------------------------------------------
// the column walk's schedule (once per tiling)
// ------------------------------------------------------------------------------------------
// one lane per CSC position: its tile's entry count (scanned afterwards into the column-walk offsets) and first slot in vals_t
__global__ void mx_csc_count_kernel(const int *__restrict__ tile_offsets, const int *__restrict__ tile_nnz_ptr, long long nt, int *__restrict__ cnt,
                                    int *__restrict__ base)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nt) return;
    const int t = tile_offsets[p];
    const int b = tile_nnz_ptr[t];
    cnt[p] = tile_nnz_ptr[t + 1] - b;
    base[p] = b;
}

// one lane per tile: (c << 4) | r of every entry in vals_t order (column-major inside the tile, rows ascending in a column)
__global__ void mx_rci_t_kernel(const uint16_t *__restrict__ masks_t, const int *__restrict__ tile_nnz_ptr, long long nt, uint8_t *__restrict__ rci_t)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    int s = tile_nnz_ptr[t];
    for (int c = 0; c < 16; ++c) {
        unsigned m = masks_t[16 * t + c];
        while (m) {
            const int r = __ffs(m) - 1;
            m &= m - 1u;
            rci_t[s++] = (uint8_t)((c << 4) | r);
        }
    }
}

pem_status pem::ensure_mx_cols(pem_ctx *ctx, const pem_tiled *A)
{
    if (A->mx_cols_ready) return PEM_OK;
    const size_t nt = (size_t)A->ntiles, nnz = (size_t)A->nnz;
    PEM_TRY(arena_phase(ctx->arena, {{&A->mx_csc_off, sizeof(int) * (nt + 4)}, {&A->mx_csc_base, sizeof(int) * (nt + 4)}, {&A->mx_rci_t, nnz + 16}}));
    PEM_TRY(A->mx_csc_off.reserve(sizeof(int) * (nt + 4)));
    PEM_TRY(A->mx_csc_base.reserve(sizeof(int) * (nt + 4)));
    PEM_TRY(A->mx_rci_t.reserve(nnz + 16));
    if (nt) {
        PEM_LAUNCH(ctx, mx_csc_count_kernel, grid_for(nt, 256), 256, A->tile_offsets.as<int>(), A->tile_nnz_ptr.as<int>(), (long long)nt,
                   A->mx_csc_off.as<int>(), A->mx_csc_base.as<int>());
        PEM_TRY(exclusive_scan_i32(ctx, A->mx_csc_off.as<int>(), A->mx_csc_off.as<int>(), nt, nullptr));
        PEM_LAUNCH(ctx, mx_rci_t_kernel, grid_for(nt, 256), 256, A->masks_t.as<uint16_t>(), A->tile_nnz_ptr.as<int>(), (long long)nt,
                   A->mx_rci_t.as<uint8_t>());
    }
    A->mx_cols_ready = true;
    return PEM_OK;
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
#define MX_NAMES(vt, k) {"mxv_kernel<" vt "," k ",rows>", "mxv_kernel<" vt "," k ",cols>"}
#define MX_NAMES_VT(vt)                                                                                                           \
    {MX_NAMES(vt, "plus_times"), MX_NAMES(vt, "min_plus"), MX_NAMES(vt, "max_plus"), MX_NAMES(vt, "max_times"),                  \
     MX_NAMES(vt, "plus_pair"), MX_NAMES(vt, "lor_land"), MX_NAMES(vt, "reduce_plus"), MX_NAMES(vt, "reduce_times"),             \
     MX_NAMES(vt, "reduce_min"), MX_NAMES(vt, "reduce_max"), MX_NAMES(vt, "reduce_lor"), MX_NAMES(vt, "reduce_land")}
static const char *const kMxNames[2][MX_KINDS][2] = {MX_NAMES_VT("float"), MX_NAMES_VT("double")};

template <typename VT, int K>
static pem_status mx_launch(pem_ctx *ctx, const pem_tiled *A, bool col, const VT *x, VT *y, int accumulate)
{
    const char *name = kMxNames[sizeof(VT) == 8][K][col];
    if (col) {
        const long long nlines = A->tile_cols;
        PEM_LAUNCH_NAMED(ctx, name, (mxv_kernel<VT, K, true>), grid_for((size_t)nlines * 64, 256), 256, A->tile_colptr.as<int>(), nlines,
                         A->mx_csc_off.as<int>(), A->mx_csc_base.as<int>(), A->tile_rowidx.as<int>(), A->mx_rci_t.as<uint8_t>(),
                         A->vals_t.as<VT>(), x, y, (long long)A->cols, accumulate);
    } else {
        const long long nlines = A->tile_rows;
        PEM_LAUNCH_NAMED(ctx, name, (mxv_kernel<VT, K, false>), grid_for((size_t)nlines * 64, 256), 256, A->tile_rowptr.as<int>(), nlines,
                         A->tile_nnz_ptr.as<int>(), (const int *)nullptr, A->tile_colidx.as<int>(), A->rowcolidx.as<uint8_t>(),
                         A->vals.as<VT>(), x, y, (long long)A->rows, accumulate);
    }
    return PEM_OK;
}

template <typename VT>
static pem_status mx_run(pem_ctx *ctx, const pem_tiled *A, int kind, bool col, const VT *x, VT *y, int accumulate)
{
    if ((col ? A->tile_cols : A->tile_rows) == 0) return PEM_OK;   // no output
    if (col) PEM_TRY(ensure_mx_cols(ctx, A));
    switch (kind) {
    case 0: return mx_launch<VT, 0>(ctx, A, col, x, y, accumulate);
    case 1: return mx_launch<VT, 1>(ctx, A, col, x, y, accumulate);
    case 2: return mx_launch<VT, 2>(ctx, A, col, x, y, accumulate);
    case 3: return mx_launch<VT, 3>(ctx, A, col, x, y, accumulate);
    case 4: return mx_launch<VT, 4>(ctx, A, col, x, y, accumulate);
    case 5: return mx_launch<VT, 5>(ctx, A, col, x, y, accumulate);
    case 6: return mx_launch<VT, 6>(ctx, A, col, x, y, accumulate);
    case 7: return mx_launch<VT, 7>(ctx, A, col, x, y, accumulate);
    case 8: return mx_launch<VT, 8>(ctx, A, col, x, y, accumulate);
    case 9: return mx_launch<VT, 9>(ctx, A, col, x, y, accumulate);
    case 10: return mx_launch<VT, 10>(ctx, A, col, x, y, accumulate);
    default: return mx_launch<VT, 11>(ctx, A, col, x, y, accumulate);
    }
}

pem_status pem::mxv_semiring(pem_ctx *ctx, const pem_tiled *A, int semiring, bool col, const float *x, float *y, int accumulate)
{
    return mx_run<float>(ctx, A, semiring, col, x, y, accumulate);
}

pem_status pem::mxv_semiring(pem_ctx *ctx, const pem_tiled *A, int semiring, bool col, const double *x, double *y, int accumulate)
{
    return mx_run<double>(ctx, A, semiring, col, x, y, accumulate);
}

static bool mx_flag_ok(int v) { return v == 0 || v == 1; }

// x: nx values (nullptr for a reduction), y: ny values, both value_bytes wide
static pem_status mx_entry(pem_ctx *ctx, const pem_tiled *A, int kind, bool col, const void *x, void *y, int accumulate, int value_bytes,
                           const char *fn)
{
    if (A->value_bytes != value_bytes) {
        set_error("%s: the tiling holds %s values; use the %s entry point", fn, A->value_bytes == 4 ? "fp32" : "fp64",
                  A->value_bytes == 4 ? "_f32" : "fp64");
        return PEM_E_INVALID;
    }
    const size_t nx = (size_t)(col ? A->rows : A->cols), ny = (size_t)(col ? A->cols : A->rows);
    if ((kind < MX_REDUCE && nx && !x) || (ny && !y)) {
        set_error("%s: null vector", fn);
        return PEM_E_INVALID;
    }
    if (kind < MX_REDUCE && nx && ny) {
        const char *xb = (const char *)x, *yb = (const char *)y;
        if (xb < yb + ny * value_bytes && yb < xb + nx * value_bytes) {
            set_error("%s: x and y overlap", fn);
            return PEM_E_INVALID;
        }
    }
    PEM_ENTER(ctx);
    if (value_bytes == 4) return mx_run<float>(ctx, A, kind, col, (const float *)x, (float *)y, accumulate);
    return mx_run<double>(ctx, A, kind, col, (const double *)x, (double *)y, accumulate);
}

static pem_status mxv_common(pem_ctx *ctx, const pem_tiled *A, int semiring, int transpose, const void *dx, void *dy, int accumulate,
                             int value_bytes, const char *fn)
{
    if (!ctx || !A) {
        set_error("%s: null context or tiling", fn);
        return PEM_E_INVALID;
    }
    if (semiring < PEM_SEMIRING_PLUS_TIMES || semiring > PEM_SEMIRING_LOR_LAND) {
        set_error("%s: unknown semiring %d (PEM_SEMIRING_PLUS_TIMES .. PEM_SEMIRING_LOR_LAND = 0 .. 5)", fn, semiring);
        return PEM_E_INVALID;
    }
    if (!mx_flag_ok(transpose) || !mx_flag_ok(accumulate)) {
        set_error("%s: transpose and accumulate must be 0 or 1 (got %d, %d)", fn, transpose, accumulate);
        return PEM_E_INVALID;
    }
    return mx_entry(ctx, A, semiring, transpose == 1, dx, dy, accumulate, value_bytes, fn);
}

static pem_status reduce_common(pem_ctx *ctx, const pem_tiled *A, int op, int dim, void *dy, int accumulate, int value_bytes, const char *fn)
{
    if (!ctx || !A) {
        set_error("%s: null context or tiling", fn);
        return PEM_E_INVALID;
    }
    if (op < PEM_BINOP_PLUS || op > PEM_BINOP_LAND) {
        set_error("%s: unknown op %d (PEM_BINOP_PLUS .. PEM_BINOP_LAND = 0 .. 5)", fn, op);
        return PEM_E_INVALID;
    }
    if (dim != PEM_REDUCE_ROWS && dim != PEM_REDUCE_COLS) {
        set_error("%s: unknown dim %d (PEM_REDUCE_ROWS = 0, PEM_REDUCE_COLS = 1)", fn, dim);
        return PEM_E_INVALID;
    }
    if (!mx_flag_ok(accumulate)) {
        set_error("%s: accumulate must be 0 or 1 (got %d)", fn, accumulate);
        return PEM_E_INVALID;
    }
    return mx_entry(ctx, A, MX_REDUCE + op, dim == PEM_REDUCE_COLS, nullptr, dy, accumulate, value_bytes, fn);
}

extern "C" pem_status pem_tiled_mxv(pem_ctx *ctx, const pem_tiled *A, int semiring, int transpose, const double *dx, double *dy, int accumulate)
{
    return mxv_common(ctx, A, semiring, transpose, dx, dy, accumulate, 8, "pem_tiled_mxv");
}

extern "C" pem_status pem_tiled_mxv_f32(pem_ctx *ctx, const pem_tiled *A, int semiring, int transpose, const float *dx, float *dy, int accumulate)
{
    return mxv_common(ctx, A, semiring, transpose, dx, dy, accumulate, 4, "pem_tiled_mxv_f32");
}

extern "C" pem_status pem_tiled_reduce(pem_ctx *ctx, const pem_tiled *A, int op, int dim, double *dy, int accumulate)
{
    return reduce_common(ctx, A, op, dim, dy, accumulate, 8, "pem_tiled_reduce");
}

extern "C" pem_status pem_tiled_reduce_f32(pem_ctx *ctx, const pem_tiled *A, int op, int dim, float *dy, int accumulate)
{
    return reduce_common(ctx, A, op, dim, dy, accumulate, 4, "pem_tiled_reduce_f32");
}
