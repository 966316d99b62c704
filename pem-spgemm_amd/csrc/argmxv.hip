// argmxv.hip -- arg folds of a tiling's rows or columns (include/pem_spgemm.h, pem_tiled_mxv_arg / pem_tiled_reduce_arg), and the
// breadth-first tree built on them (pem_tiled_bfs_parents): where a minimum or maximum was attained, next to -- or instead of -- its
// value.
//
// The walk is frontier_kernel's (frontier.hip): one wave per line, chunks of 64 entries, the presence words, the line flags, the
// allowed-output bits, the early return for a line nothing can reach, ALLX for a dense x.  What it adds is the x-index of every live
// entry, 16 * the tile's minor index + the entry's minor: the column j for rows, the row i for columns.
//   value kinds  (min_plus, max_plus, max_times, and the reductions with the x gather compiled out)  the term goes into the wave's LDS
//          at the entry's slot of the chunk regrouped by major, as in mxv.hip, and the x-index into a second array at the same slot,
//          1 KB per block.  The lane that owns the output chains both: the accumulator moves by pem_fmin / pem_fmax exactly as
//          frontier_kernel's, and whenever it moves (next != acc) the term's index goes along -- the compare hangs off the chain, not
//          on it.  A fresh fold starts from NaN, not from +-inf, so that its first non-NaN term moves it whatever it is (an infinite
//          term is a term); a fold that ends on NaN had no winner and writes the start value and -1.  The entries of one major
//          ascend in the x-index inside a chunk and from chunk to chunk, and a later term that merely equals the best (+0 and -0
//          included) does not move the accumulator: the index reported is the smallest among the equal best, whatever chunk they
//          sit in.
//   index kinds  (min_index, max_index)  no value is loaded and nothing is staged: the first (last) lane of a major's ballot holds the
//          major's smallest (largest) x-index of the chunk, and the owning lane fetches it with one shuffle.
// One walk: A's entries are read once.  No atomics: every y, idx and presence byte is written by the one lane that folded it.
#include "spgemm_internal.h"
#include "tiled_internal.h"
#include "mx_internal.h"
#include <climits>

using namespace pem;

// the kinds: pem_arg_kind, then the two reductions (terms are the stored values: no x)
enum { ARG_REDUCE_MIN = 5, ARG_REDUCE_MAX = 6, ARG_KINDS = 7 };

template <int AK>
struct ArgOp {
    static constexpr bool index_only = AK == PEM_ARG_MIN_INDEX || AK == PEM_ARG_MAX_INDEX;
    static constexpr bool is_min = AK == PEM_ARG_MIN_PLUS || AK == PEM_ARG_MIN_INDEX || AK == ARG_REDUCE_MIN;
    static constexpr bool reads_vals = !index_only;
    static constexpr bool reads_x = AK <= PEM_ARG_MAX_TIMES;
    // the fold of mx_internal.h whose term and step these are
    static constexpr int mx = AK == PEM_ARG_MIN_PLUS    ? PEM_SEMIRING_MIN_PLUS
                              : AK == PEM_ARG_MAX_PLUS  ? PEM_SEMIRING_MAX_PLUS
                              : AK == PEM_ARG_MAX_TIMES ? PEM_SEMIRING_MAX_TIMES
                              : is_min                  ? MX_REDUCE + PEM_BINOP_MIN
                                                        : MX_REDUCE + PEM_BINOP_MAX;
    using Mx = MxOp<mx>;
    // one chain step: the accumulator moves as frontier_kernel's (a NaN side is skipped); the index follows it when it moves -- t is
    // strictly better, or acc was NaN.  (While acc is NaN a NaN term leaves a stale index: the end of the walk drops it.)
    template <typename VT> static __device__ __forceinline__ void step(VT &acc, int &best, VT t, int i)
    {
        const VT next = Mx::template step<VT>(acc, t, VT(0));
        if (!(next == acc)) best = i;
        acc = next;
    }
};

// frontier_kernel's arguments, and idx: the x-index of the winning term per output.  y, vals and x are unread under the index kinds
// (VT is float there), x under the reductions.
template <typename VT, int AK, bool COL, bool ALLX>
__global__ void __launch_bounds__(256) arg_kernel(const int *__restrict__ lptr, long long nlines, const int *__restrict__ poff,
                                                  const int *__restrict__ pbase, const int *__restrict__ pminor, const uint8_t *__restrict__ rci,
                                                  const VT *__restrict__ vals, const VT *__restrict__ x, const uint16_t *__restrict__ words,
                                                  const uint8_t *__restrict__ line_flag, VT *__restrict__ y, int *__restrict__ idx, long long nout,
                                                  const uint8_t *__restrict__ mask, int complement, uint8_t *__restrict__ ypres, int accumulate)
{
    using Op = ArgOp<AK>;
    __shared__ VT s_t[Op::index_only ? 1 : 4 * 64];    // [wave][slot]: the entry's term
    __shared__ int s_i[Op::index_only ? 1 : 4 * 64];   // [wave][slot]: the entry's x-index
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long L = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (L >= nlines) return;   // (wave-uniform)
    VT *const my_t = s_t + (Op::index_only ? 0 : wv * 64);
    int *const my_i = s_i + (Op::index_only ? 0 : wv * 64);
    const long long o = 16 * L + lane;
    const bool out_lane = lane < 16 && o < nout;
    bool allowed = out_lane;
    if (out_lane && mask) allowed = (mask[o] != 0) != (complement != 0);
    const unsigned allowed_bits = (unsigned)__ballot(allowed);
    bool flagged = true;
    if constexpr (!ALLX) flagged = line_flag[L] != 0;
    if (!flagged || allowed_bits == 0u) {   // (wave-uniform) nothing can enter a fold of this line
        if (allowed && !accumulate) {
            if constexpr (!Op::index_only) y[o] = Op::Mx::template start<VT>();
            idx[o] = -1;
        }
        if (out_lane && ypres) ypres[o] = 0;
        return;
    }
    VT acc = VT(__builtin_nanf(""));   // a fresh fold: the first non-NaN term moves it (header comment)
    int best = -1;
    if (allowed && accumulate) {
        if constexpr (Op::index_only) {
            best = idx[o];
            if (best < 0) best = -1;
        } else {
            acc = y[o];
        }
    }
    int touched = 0;
    const int p0 = lptr[L], p1 = lptr[L + 1];
    if (p0 < p1) {
        const int e_end = poff[p1];
        int pc = p0;
        for (int eb = poff[p0]; eb < e_end; eb += 64) {   // wave-uniform trip count
            const int mp = pc + lane;
            const bool lv = mp < p1;
            const int my_off = lv ? poff[mp] : INT_MAX;
            const int my_minor = lv ? pminor[mp] : 0;
            unsigned my_word = 0xFFFFu;
            if constexpr (!ALLX) my_word = lv ? words[my_minor] : 0u;
            int my_base = 0;
            if constexpr (COL) my_base = lv ? pbase[mp] : 0;
            const int e = eb + lane;
            const int ti = chunk_tile_of(my_off, e);
            const int t_off = __shfl(my_off, ti, 64), t_minor = __shfl(my_minor, ti, 64);
            const unsigned t_word = (unsigned)__shfl((int)my_word, ti, 64);
            int t_base = 0;
            if constexpr (COL) t_base = __shfl(my_base, ti, 64);
            const int ti_last = __shfl(ti, 63, 64);
            int major = 16, xi = 0;
            VT a = VT(0), xv = VT(0);
            if (e < e_end && t_word != 0u) {
                const int slot = COL ? t_base + (e - t_off) : e;
                const unsigned rc = rci[slot];
                if (((t_word >> (rc & 15u)) & (allowed_bits >> (rc >> 4)) & 1u) != 0u) {   // live
                    major = (int)(rc >> 4);
                    xi = 16 * t_minor + (int)(rc & 15u);
                    if constexpr (Op::reads_vals) a = vals[slot];
                    if constexpr (Op::reads_x) xv = x[(size_t)xi];
                }
            }
            if (__ballot(major < 16) != 0ull) {   // (wave-uniform) a chunk without a live entry stages and chains nothing
                if constexpr (Op::index_only) {
                    // the entries of a major ascend in the x-index with the lane: its first (last) lane holds the chunk's candidate
                    int src = 0, have = 0;
#pragma unroll
                    for (int m = 0; m < 16; ++m) {
                        const unsigned long long b = __ballot(major == m);
                        if (lane == m && b != 0ull) {
                            have = 1;
                            src = Op::is_min ? __ffsll((long long)b) - 1 : 63 - __clzll((long long)b);
                        }
                    }
                    const int cand = __shfl(xi, src, 64);
                    if (have) best = best < 0 ? cand : (Op::is_min ? min(best, cand) : max(best, cand));
                    touched |= have;
                } else {
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
                    mx_wave_sync();   // the previous staged chunk's chain has read the staging area
                    if (major < 16) {
                        my_t[slot] = Op::Mx::template term<VT>(a, xv);
                        my_i[slot] = xi;
                    }
                    mx_wave_sync();
                    touched |= my_cnt;
                    const VT *pt = my_t + my_first;
                    const int *pi = my_i + my_first;
                    int k = 0;
                    for (; k + 4 <= my_cnt; k += 4) {   // four reads ahead of the chain
                        const VT t0 = pt[k], t1 = pt[k + 1], t2 = pt[k + 2], t3 = pt[k + 3];
                        const int i0 = pi[k], i1 = pi[k + 1], i2 = pi[k + 2], i3 = pi[k + 3];
                        Op::template step<VT>(acc, best, t0, i0);
                        Op::template step<VT>(acc, best, t1, i1);
                        Op::template step<VT>(acc, best, t2, i2);
                        Op::template step<VT>(acc, best, t3, i3);
                    }
                    for (; k < my_cnt; ++k) Op::template step<VT>(acc, best, pt[k], pi[k]);
                }
            }
            // the next chunk starts in the tile of entry eb + 63, or in the one after it
            int pn = pc + ti_last;
            if (eb + 64 < e_end && pn + 1 < p1 && poff[pn + 1] <= eb + 64) ++pn;
            pc = pn;
        }
    }
    if constexpr (Op::index_only) {
        if (allowed && (touched || !accumulate)) idx[o] = best;
    } else {
        const bool real = acc == acc, won = real && best >= 0;   // (a fold still on NaN had no winner)
        if (allowed && !accumulate) {
            y[o] = real ? acc : Op::Mx::template start<VT>();
            idx[o] = won ? best : -1;
        } else if (allowed) {
            if (touched) y[o] = acc;
            if (won) idx[o] = best;
        }
    }
    if (out_lane && ypres) ypres[o] = (allowed && touched) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
#define ARG_NAMES(vt, k)                                                                                                                 \
    {{"arg_kernel<" vt "," k ",rows>", "arg_kernel<" vt "," k ",rows,allx>"}, {"arg_kernel<" vt "," k ",cols>", "arg_kernel<" vt "," k ",cols,allx>"}}
#define ARG_NAMES_VT(vt)                                                                                                                 \
    {ARG_NAMES(vt, "min_plus"), ARG_NAMES(vt, "max_plus"), ARG_NAMES(vt, "max_times"), ARG_NAMES(vt, "min_index"), ARG_NAMES(vt, "max_index"), \
     ARG_NAMES(vt, "reduce_min"), ARG_NAMES(vt, "reduce_max")}
static const char *const kArgNames[2][ARG_KINDS][2][2] = {ARG_NAMES_VT("float"), ARG_NAMES_VT("double")};

namespace {

struct ArgArgs {
    const void *x;
    const uint8_t *xpres;
    void *y;
    int *idx;
    const uint8_t *mask;
    int complement;
    uint8_t *ypres;
    int accumulate;
};

template <typename VT, int AK, bool COL, bool ALLX>
void arg_launch_walk(pem_ctx *ctx, const pem_tiled *A, const ArgArgs &f, const uint16_t *words, const uint8_t *flags)
{
    const char *name = kArgNames[sizeof(VT) == 8][AK][COL][ALLX];
    const VT *x = (const VT *)f.x;
    VT *y = (VT *)f.y;
    if constexpr (COL) {
        const long long nlines = A->tile_cols;
        PEM_LAUNCH_NAMED(ctx, name, (arg_kernel<VT, AK, true, ALLX>), grid_for((size_t)nlines * 64, 256), 256, A->tile_colptr.as<int>(), nlines,
                         A->mx_csc_off.as<int>(), A->mx_csc_base.as<int>(), A->tile_rowidx.as<int>(), A->mx_rci_t.as<uint8_t>(),
                         A->vals_t.as<VT>(), x, words, flags, y, f.idx, (long long)A->cols, f.mask, f.complement, f.ypres, f.accumulate);
    } else {
        const long long nlines = A->tile_rows;
        PEM_LAUNCH_NAMED(ctx, name, (arg_kernel<VT, AK, false, ALLX>), grid_for((size_t)nlines * 64, 256), 256, A->tile_rowptr.as<int>(), nlines,
                         A->tile_nnz_ptr.as<int>(), (const int *)nullptr, A->tile_colidx.as<int>(), A->rowcolidx.as<uint8_t>(),
                         A->vals.as<VT>(), x, words, flags, y, f.idx, (long long)A->rows, f.mask, f.complement, f.ypres, f.accumulate);
    }
}

template <typename VT, int AK>
void arg_launch(pem_ctx *ctx, const pem_tiled *A, bool col, const ArgArgs &f, const uint16_t *words, const uint8_t *flags)
{
    if constexpr (AK >= ARG_REDUCE_MIN) {   // the reductions: a dense walk only
        if (col) arg_launch_walk<VT, AK, true, true>(ctx, A, f, words, flags);
        else arg_launch_walk<VT, AK, false, true>(ctx, A, f, words, flags);
    } else if (col) {
        if (f.xpres) arg_launch_walk<VT, AK, true, false>(ctx, A, f, words, flags);
        else arg_launch_walk<VT, AK, true, true>(ctx, A, f, words, flags);
    } else {
        if (f.xpres) arg_launch_walk<VT, AK, false, false>(ctx, A, f, words, flags);
        else arg_launch_walk<VT, AK, false, true>(ctx, A, f, words, flags);
    }
}

// the call for checked arguments, inside PEM_ENTER: pack and mark (fr_prepare), walk.  Stream-ordered, no read-back.  The index
// kinds read no value: one instantiation serves both value types.
template <typename VT>
pem_status arg_run(pem_ctx *ctx, const pem_tiled *A, int ak, bool col, const ArgArgs &f)
{
    const long long nlines = col ? A->tile_cols : A->tile_rows;
    ctx->fr_lines = f.xpres ? nlines : -1;
    if (nlines == 0) return PEM_OK;   // no output
    const uint16_t *words = nullptr;
    const uint8_t *flags = nullptr;
    PEM_TRY(fr_prepare(ctx, A, col, f.xpres, &words, &flags));
    switch (ak) {
    case PEM_ARG_MIN_PLUS: arg_launch<VT, PEM_ARG_MIN_PLUS>(ctx, A, col, f, words, flags); break;
    case PEM_ARG_MAX_PLUS: arg_launch<VT, PEM_ARG_MAX_PLUS>(ctx, A, col, f, words, flags); break;
    case PEM_ARG_MAX_TIMES: arg_launch<VT, PEM_ARG_MAX_TIMES>(ctx, A, col, f, words, flags); break;
    case PEM_ARG_MIN_INDEX: arg_launch<float, PEM_ARG_MIN_INDEX>(ctx, A, col, f, words, flags); break;
    case PEM_ARG_MAX_INDEX: arg_launch<float, PEM_ARG_MAX_INDEX>(ctx, A, col, f, words, flags); break;
    case ARG_REDUCE_MIN: arg_launch<VT, ARG_REDUCE_MIN>(ctx, A, col, f, words, flags); break;
    default: arg_launch<VT, ARG_REDUCE_MAX>(ctx, A, col, f, words, flags); break;
    }
    return PEM_OK;
}

bool arg_value_type_ok(const pem_tiled *A, int vb, const char *fn)
{
    if (A->value_bytes == vb) return true;
    set_error("%s: the tiling holds %s values; use the %s entry point", fn, A->value_bytes == 4 ? "fp32" : "fp64",
              A->value_bytes == 4 ? "_f32" : "fp64");
    return false;
}

pem_status arg_common(pem_ctx *ctx, const pem_tiled *A, int kind, int transpose, const void *dx, const uint8_t *dx_present, void *dy,
                      int32_t *d_idx, const uint8_t *dy_mask, int mask_complement, uint8_t *dy_present, int accumulate, int vb, const char *fn)
{
    if (!ctx || !A) {
        set_error("%s: null context or tiling", fn);
        return PEM_E_INVALID;
    }
    if (kind < PEM_ARG_MIN_PLUS || kind > PEM_ARG_MAX_INDEX) {
        set_error("%s: unknown kind %d (PEM_ARG_MIN_PLUS .. PEM_ARG_MAX_INDEX = 0 .. 4)", fn, kind);
        return PEM_E_INVALID;
    }
    if (!fr_flag_ok(transpose) || !fr_flag_ok(accumulate) || !fr_flag_ok(mask_complement)) {
        set_error("%s: transpose, accumulate and mask_complement must be 0 or 1 (got %d, %d, %d)", fn, transpose, accumulate, mask_complement);
        return PEM_E_INVALID;
    }
    if (!arg_value_type_ok(A, vb, fn)) return PEM_E_INVALID;
    if (!d_idx) {
        set_error("%s: null d_idx", fn);
        return PEM_E_INVALID;
    }
    const bool col = transpose == 1, values = kind <= PEM_ARG_MAX_TIMES;
    const size_t nx = (size_t)(col ? A->rows : A->cols), ny = (size_t)(col ? A->cols : A->rows);
    if (values && ((nx && !dx) || (ny && !dy))) {
        set_error("%s: null vector", fn);
        return PEM_E_INVALID;
    }
    if (!values) dx = dy = nullptr;   // neither read nor written: their bytes are nobody's business
    const Span sx(dx, nx * vb), sy(dy, ny * vb), sxp(dx_present, nx), sm(dy_mask, ny), syp(dy_present, ny), si(d_idx, ny * sizeof(int32_t));
    if (sx.meets(sy)) {
        set_error("%s: x and y overlap", fn);
        return PEM_E_INVALID;
    }
    if (syp.meets(sm) || syp.meets(sxp) || syp.meets(sx) || syp.meets(sy)) {
        set_error("%s: dy_present overlaps %s", fn, syp.meets(sm) ? "dy_mask" : syp.meets(sxp) ? "dx_present" : syp.meets(sx) ? "x" : "y");
        return PEM_E_INVALID;
    }
    if (si.meets(sx) || si.meets(sy) || si.meets(sxp) || si.meets(sm) || si.meets(syp)) {
        set_error("%s: d_idx overlaps %s", fn,
                  si.meets(sx) ? "x" : si.meets(sy) ? "y" : si.meets(sxp) ? "dx_present" : si.meets(sm) ? "dy_mask" : "dy_present");
        return PEM_E_INVALID;
    }
    PEM_ENTER(ctx);
    const ArgArgs f{dx, dx_present, dy, d_idx, dy_mask, mask_complement, dy_present, accumulate};
    return vb == 4 ? arg_run<float>(ctx, A, kind, col, f) : arg_run<double>(ctx, A, kind, col, f);
}

pem_status reduce_arg_common(pem_ctx *ctx, const pem_tiled *A, int op, int dim, void *dy, int32_t *d_idx, int vb, const char *fn)
{
    if (!ctx || !A) {
        set_error("%s: null context or tiling", fn);
        return PEM_E_INVALID;
    }
    if (op != PEM_BINOP_MIN && op != PEM_BINOP_MAX) {
        set_error("%s: unknown op %d (PEM_BINOP_MIN = 2, PEM_BINOP_MAX = 3)", fn, op);
        return PEM_E_INVALID;
    }
    if (dim != PEM_REDUCE_ROWS && dim != PEM_REDUCE_COLS) {
        set_error("%s: unknown dim %d (PEM_REDUCE_ROWS = 0, PEM_REDUCE_COLS = 1)", fn, dim);
        return PEM_E_INVALID;
    }
    if (!arg_value_type_ok(A, vb, fn)) return PEM_E_INVALID;
    if (!d_idx) {
        set_error("%s: null d_idx", fn);
        return PEM_E_INVALID;
    }
    const bool col = dim == PEM_REDUCE_COLS;
    const size_t ny = (size_t)(col ? A->cols : A->rows);
    if (ny && !dy) {
        set_error("%s: null vector", fn);
        return PEM_E_INVALID;
    }
    if (Span(d_idx, ny * sizeof(int32_t)).meets(Span(dy, ny * vb))) {
        set_error("%s: d_idx overlaps y", fn);
        return PEM_E_INVALID;
    }
    PEM_ENTER(ctx);
    const ArgArgs f{nullptr, nullptr, dy, d_idx, nullptr, 0, nullptr, 0};
    const int ak = op == PEM_BINOP_MIN ? ARG_REDUCE_MIN : ARG_REDUCE_MAX;
    return vb == 4 ? arg_run<float>(ctx, A, ak, col, f) : arg_run<double>(ctx, A, ak, col, f);
}

}  // namespace

extern "C" pem_status pem_tiled_mxv_arg(pem_ctx *ctx, const pem_tiled *A, int kind, int transpose, const double *dx, const uint8_t *dx_present,
                                        double *dy, int32_t *d_idx, const uint8_t *dy_mask, int mask_complement, uint8_t *dy_present,
                                        int accumulate)
{
    return arg_common(ctx, A, kind, transpose, dx, dx_present, dy, d_idx, dy_mask, mask_complement, dy_present, accumulate, 8, "pem_tiled_mxv_arg");
}

extern "C" pem_status pem_tiled_mxv_arg_f32(pem_ctx *ctx, const pem_tiled *A, int kind, int transpose, const float *dx, const uint8_t *dx_present,
                                            float *dy, int32_t *d_idx, const uint8_t *dy_mask, int mask_complement, uint8_t *dy_present,
                                            int accumulate)
{
    return arg_common(ctx, A, kind, transpose, dx, dx_present, dy, d_idx, dy_mask, mask_complement, dy_present, accumulate, 4,
                      "pem_tiled_mxv_arg_f32");
}

extern "C" pem_status pem_tiled_reduce_arg(pem_ctx *ctx, const pem_tiled *A, int op, int dim, double *dy, int32_t *d_idx)
{
    return reduce_arg_common(ctx, A, op, dim, dy, d_idx, 8, "pem_tiled_reduce_arg");
}

extern "C" pem_status pem_tiled_reduce_arg_f32(pem_ctx *ctx, const pem_tiled *A, int op, int dim, float *dy, int32_t *d_idx)
{
    return reduce_arg_common(ctx, A, op, dim, dy, d_idx, 4, "pem_tiled_reduce_arg_f32");
}

// ------------------------------------------------------------------------------------------
// breadth-first search with parents
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) bfsp_init_kernel(long long n, long long source, int *__restrict__ level, int *__restrict__ parent,
                                                        uint8_t *__restrict__ visited, uint8_t *__restrict__ frontier)
{
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const bool s = v == source;
    level[v] = s ? 0 : -1;
    parent[v] = s ? (int)source : -1;
    visited[v] = s;
    frontier[v] = s;
}

// after a level's walk: the new vertices get their level and join visited; found is raised by a plain store of one value
__global__ void __launch_bounds__(256) bfsp_level_kernel(long long n, const uint8_t *__restrict__ next, int lvl, int *__restrict__ level,
                                                         uint8_t *__restrict__ visited, int *__restrict__ found)
{
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n || !next[v]) return;
    level[v] = lvl;
    visited[v] = 1;
    *found = 1;
}

// one workgroup: the number of visited vertices
__global__ void __launch_bounds__(1024) bfsp_count_kernel(long long n, const uint8_t *__restrict__ visited, long long *__restrict__ out)
{
    __shared__ long long part[16];
    long long c = 0;
    for (long long v = threadIdx.x; v < n; v += 1024) c += visited[v] != 0;
    for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long t = 0;
        for (int w = 0; w < 16; ++w) t += part[w];
        *out = t;
    }
}

extern "C" pem_status pem_tiled_bfs_parents(pem_ctx *ctx, const pem_tiled *A, int64_t source, int transpose, int32_t *d_level, int32_t *d_parent,
                                            int32_t *depth, int64_t *reached)
{
    const char *fn = "pem_tiled_bfs_parents";
    if (!ctx || !A || !d_level || !d_parent || !depth || !reached) {
        set_error("%s: null argument", fn);
        return PEM_E_INVALID;
    }
    if (!fr_flag_ok(transpose)) {
        set_error("%s: transpose must be 0 or 1 (got %d)", fn, transpose);
        return PEM_E_INVALID;
    }
    if (A->rows != A->cols) {
        set_error("%s: the tiling is %d x %d; a search needs a square one", fn, A->rows, A->cols);
        return PEM_E_INVALID;
    }
    if (source < 0 || source >= A->rows) {
        set_error("%s: source %lld outside [0, %d)", fn, (long long)source, A->rows);
        return PEM_E_INVALID;
    }
    if (Span(d_level, (size_t)A->rows * sizeof(int32_t)).meets(Span(d_parent, (size_t)A->rows * sizeof(int32_t)))) {
        set_error("%s: d_level and d_parent overlap", fn);
        return PEM_E_INVALID;
    }
    PEM_ENTER(ctx);
    const long long n = A->rows;
    const size_t nb = ((size_t)n + 255) & ~size_t(255);
    // visited, two frontiers, the found word and the count
    DevBuf work;
    PEM_TRY(work.reserve(3 * nb + 256));
    uint8_t *visited = work.as<uint8_t>(), *cur = visited + nb, *next = cur + nb;
    int *found = reinterpret_cast<int *>(next + nb);
    long long *count = reinterpret_cast<long long *>(next + nb + 8);
    PEM_LAUNCH(ctx, bfsp_init_kernel, grid_for((size_t)n, 256), 256, n, (long long)source, d_level, d_parent, visited, cur);
    int lvl = 0;
    bool any = false;   // the last level found new vertices
    int *const h_found = reinterpret_cast<int *>(ctx->h_scalars);
    for (;;) {
        ++lvl;
        PEM_HIP(hipMemsetAsync(found, 0, sizeof(int), ctx->stream));
        // the unvisited ends of the frontier's edges get the least frontier vertex with an edge to them: A^T.f follows the edges
        // forwards, A.f backwards; accumulate = 1 (every unvisited parent is -1) keeps the lines nothing reaches from writing
        const ArgArgs f{nullptr, cur, nullptr, d_parent, visited, 1, next, 1};
        PEM_TRY(arg_run<float>(ctx, A, PEM_ARG_MIN_INDEX, transpose == 0, f));
        PEM_LAUNCH(ctx, bfsp_level_kernel, grid_for((size_t)n, 256), 256, n, next, lvl, d_level, visited, found);
        PEM_TRY(launch_status(ctx));
        PEM_HIP(hipMemcpyAsync(h_found, found, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        PEM_HIP(hipStreamSynchronize(ctx->stream));
        any = *h_found != 0;
        if (!any || lvl >= n) break;
        uint8_t *t = cur;
        cur = next;
        next = t;
    }
    PEM_LAUNCH(ctx, bfsp_count_kernel, 1, 1024, n, visited, count);
    int64_t c = 0;
    PEM_TRY(read_scalars(ctx, reinterpret_cast<const int64_t *>(count), 1, &c));
    PEM_TRY(launch_status(ctx));
    *depth = any ? lvl : lvl - 1;
    *reached = c;
    return PEM_OK;
}
