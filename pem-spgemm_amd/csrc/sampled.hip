// sampled.hip -- the sampled sparse product (include/pem_spgemm.h, pem_tiled_sampled_mxm / pem_tiled_set_values_sampled_mxm): the
// values of a tiling become R(i, j) = (+)_k A(i, k) (x) B(k, j) (transpose_b: B(j, k)) at the tiling's own stored positions, the
// fold running over the k both operands store, in ascending k, with step 3's arithmetic (the SR policies of spgemm_internal.h).
// A dot-product method: nothing of A * B outside the pattern is ever listed, so the cost follows the pattern and the tile lists
// it touches, not flop(A * B).  The pattern is never touched and the old values are read only under accumulate.
//
// The work unit is one tile (ti, tj) of the pattern, taken by a group of LPT lanes (64: one wave per tile, 16: four tiles per
// wave).  Two lists meet there: A's tile row ti (tile ids tile_rowptr[ti] .., keys tile_colidx) and B's tile column tj (positions
// tile_colptr[tj] .., keys tile_rowidx, tile ids tile_offsets) -- under transpose_b B's tile row tj, read exactly as A's.  Both
// are ascending.  The group walks the shorter list LPT keys at a time, one key per lane, each lane binary-searches its key in the
// longer list, the hits are balloted and consumed from the low bit up: the matched tile pairs arrive in ascending inner tile
// index, which is step 3's pair order.  For a matched pair (ta, tb) a lane holding the pattern entry (r, c) reads A's record of
// row r, tile_rec[16 ta + r], and B's record of column c -- tile_rec_t[16 tb + c] with values in vals_t, or under transpose_b
// tile_rec[16 tb + c] with values in vals: a tile's row-side record and row-major values ARE the column-side record and
// column-major values of its transpose, so one body serves both through SmSide.  The lane walks the set bits of maskA & maskB in
// ascending order and addresses each operand with the record's prefix count plus a popcount of the lower mask bits, as
// s3_accumulate_wide_kernel does (step3.hip).  A lane owns entries gl, gl + LPT, ... of its tile, 256 / LPT accumulators at
// most, all in registers.  Every value is written once, to vals and through vmap_t (values.hip) to vals_t: no atomics.
// The pair lists are not kept: a refresh searches again, which is what keeps it allocation-free.
#include "spgemm_internal.h"
#include "tiled_internal.h"
#include "mx_internal.h"
#include <cstdlib>

using namespace pem;

namespace {

template <int K> struct SmSr;
template <> struct SmSr<PEM_SEMIRING_PLUS_TIMES> { using type = SrPlusTimes; };
template <> struct SmSr<PEM_SEMIRING_MIN_PLUS> { using type = SrMinPlus; };
template <> struct SmSr<PEM_SEMIRING_MAX_PLUS> { using type = SrMaxPlus; };
template <> struct SmSr<PEM_SEMIRING_MAX_TIMES> { using type = SrMaxTimes; };
template <> struct SmSr<PEM_SEMIRING_PLUS_PAIR> { using type = SrPlusPair; };
template <> struct SmSr<PEM_SEMIRING_LOR_LAND> { using type = SrLorLand; };

// one operand as the kernel reads it: list l is positions ptr[l] .. ptr[l + 1], ascending in key; position p is tile tid[p] (null:
// p itself); line q (0 .. 15) of tile t has the record rec[16 t + q] = mask | entries of the lines before << 16, and its stored
// values sit from vals[nnz_ptr[t] + (rec >> 16)] in ascending inner index
template <typename VT>
struct SmSide {
    const int *ptr, *key, *tid, *nnz_ptr;
    const uint32_t *rec;
    const VT *vals;
};

}   // namespace

// s_keys[t] = tile row << 32 | tile column of pattern tile t; s_ptr[t .. t + 1]: its entries; s_rci: (r << 4) | c per entry.
// vals_t null: only vals is written (the builder derives vals_t afterwards).
template <typename VT, int K, int LPT>
__global__ void __launch_bounds__(256) sampled_kernel(const long long *__restrict__ s_keys, const int *__restrict__ s_ptr,
                                                      const uint8_t *__restrict__ s_rci, long long nt, const SmSide<VT> A, const SmSide<VT> B,
                                                      int accumulate, VT *vals, const int *__restrict__ vmap_t, VT *vals_t)
{
    using SR = typename SmSr<K>::type;
    constexpr int G = 64 / LPT;       // pattern tiles per wave
    constexpr int NACC = 256 / LPT;   // entries a lane may own
    const int lane = threadIdx.x & 63, gl = lane % LPT, gb = lane - gl;
    const long long nwaves = (long long)gridDim.x * (blockDim.x >> 6);
    const long long nwork = (nt + G - 1) / G;
    for (long long w = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6; w < nwork; w += nwaves) {   // wave-uniform
        const long long t = w * G + lane / LPT;
        int e0 = 0, ne = 0, a0 = 0, la = 0, b0 = 0, lb = 0;
        if (t < nt) {
            const long long key = s_keys[t];
            const int ti = (int)(key >> 32), tj = (int)(key & 0xFFFFFFFFll);
            e0 = s_ptr[t];
            ne = s_ptr[t + 1] - e0;
            a0 = A.ptr[ti];
            la = A.ptr[ti + 1] - a0;
            b0 = B.ptr[tj];
            lb = B.ptr[tj + 1] - b0;
        }
        if (la == 0 || lb == 0) la = lb = 0;   // an empty side: nothing is searched
        const bool walk_b = lb < la;           // the shorter list is walked, the longer one searched
        const int *const skey = walk_b ? B.key + b0 : A.key + a0;
        const int *const lkey = walk_b ? A.key + a0 : B.key + b0;
        const int ns = walk_b ? lb : la, nl = walk_b ? la : lb;
        int nemax = ne, nsmax = ns;            // over the wave's groups (wave-uniform trip counts)
#pragma unroll
        for (int g = 1; g < G; ++g) {
            nemax = max(nemax, __shfl(ne, (gb + g * LPT) & 63, 64));
            nsmax = max(nsmax, __shfl(ns, (gb + g * LPT) & 63, 64));
        }
        unsigned rc[NACC];
        VT acc[NACC];
#pragma unroll
        for (int i = 0; i < NACC; ++i) {
            const int e = i * LPT + gl;
            rc[i] = 0;
            acc[i] = SR::template start<VT>();
            if (e < ne) {
                rc[i] = s_rci[e0 + e];
                if (accumulate) acc[i] = MxOp<K>::template from_y<VT>(vals[e0 + e]);
            }
        }
        for (int base = 0; base < nsmax; base += LPT) {
            // 1. the chunk's keys, one per lane, searched in the longer list
            const int si = base + gl;
            int lpos = -1;
            if (si < ns) {
                const int k = skey[si];
                int lo = 0, hi = nl;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (lkey[mid] < k)
                        lo = mid + 1;
                    else
                        hi = mid;
                }
                if (lo < nl && lkey[lo] == k) lpos = lo;
            }
            unsigned long long hits = __ballot(lpos >= 0);
            if constexpr (LPT < 64) hits = (hits >> gb) & ((1ull << LPT) - 1ull);
            // 2. the matched tile pairs in ascending inner tile index
            while (__any(hits != 0ull)) {
                const int bit = hits ? __builtin_ctzll(hits) : 0;
                const int lp = __shfl(lpos, gb + bit, 64);
                if (hits) {
                    const int sp = base + bit;
                    const int ap = a0 + (walk_b ? lp : sp), bp = b0 + (walk_b ? sp : lp);
                    const int ta = A.tid ? A.tid[ap] : ap, tb = B.tid ? B.tid[bp] : bp;
                    int ao = 0, bo = 0;
                    if constexpr (SR::vals) {
                        ao = A.nnz_ptr[ta];
                        bo = B.nnz_ptr[tb];
                    }
#pragma unroll
                    for (int i = 0; i < NACC; ++i) {
                        if (i * LPT >= nemax) break;   // (wave-uniform)
                        if (i * LPT + gl < ne) {
                            const unsigned aw = A.rec[16 * (size_t)ta + (rc[i] >> 4)], bw = B.rec[16 * (size_t)tb + (rc[i] & 15u)];
                            const unsigned am = aw & 0xFFFFu, bm = bw & 0xFFFFu;
                            unsigned m = am & bm;
                            if constexpr (!SR::vals) {
                                acc[i] = SR::template count<VT>(m, acc[i]);
                            } else {
                                const VT *const av = A.vals + ao + (int)(aw >> 16), *const bv = B.vals + bo + (int)(bw >> 16);
                                while (m) {
                                    const int kk = __builtin_ctz(m);
                                    m &= m - 1;
                                    const unsigned below = (1u << kk) - 1u;
                                    acc[i] = SR::template combine<VT>(av[__popc(am & below)], bv[__popc(bm & below)], acc[i]);
                                }
                            }
                        }
                    }
                }
                hits &= hits - 1ull;
            }
        }
#pragma unroll
        for (int i = 0; i < NACC; ++i) {
            const int e = i * LPT + gl;
            if (e < ne) {
                vals[e0 + e] = acc[i];
                if (vals_t) vals_t[vmap_t[e0 + e]] = acc[i];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
#define SM_NAMES(vt, s) {"sampled_kernel<" vt "," s ",64>", "sampled_kernel<" vt "," s ",16>"}
#define SM_NAMES_VT(vt) \
    {SM_NAMES(vt, "plus_times"), SM_NAMES(vt, "min_plus"), SM_NAMES(vt, "max_plus"), SM_NAMES(vt, "max_times"), SM_NAMES(vt, "plus_pair"), \
     SM_NAMES(vt, "lor_land")}
static const char *const kSmNames[2][6][2] = {SM_NAMES_VT("float"), SM_NAMES_VT("double")};

// lanes per pattern tile: SM_LPT_DEFAULT unless PEM_SAMPLED_LPT (a measurement knob, read at every call) says 16 or 64
enum { SM_LPT_DEFAULT = 64 };
static int sm_lanes_per_tile()
{
    const char *e = getenv("PEM_SAMPLED_LPT");
    const int v = e ? atoi(e) : 0;
    return v == 16 || v == 64 ? v : SM_LPT_DEFAULT;
}

// the most blocks of a launch: the waves stride over the pattern's tiles past that (64-bit work indices throughout)
static constexpr size_t kSmMaxBlocks = size_t(1) << 22;

template <typename VT>
static SmSide<VT> sm_row_side(const pem_tiled *T)
{
    return {T->tile_rowptr.as<int>(), T->tile_colidx.as<int>(), nullptr, T->tile_nnz_ptr.as<int>(), T->tile_rec.as<uint32_t>(), T->vals.as<VT>()};
}
template <typename VT>
static SmSide<VT> sm_col_side(const pem_tiled *T)
{
    return {T->tile_colptr.as<int>(), T->tile_rowidx.as<int>(), T->tile_offsets.as<int>(), T->tile_nnz_ptr.as<int>(), T->tile_rec_t.as<uint32_t>(),
            T->vals_t.as<VT>()};
}

// S gives the pattern, the values go to vals and (unless null) through vmap_t to vals_t
template <typename VT, int K>
static void sm_launch(pem_ctx *ctx, const pem_tiled *S, const pem_tiled *A, const pem_tiled *B, int transpose_b, int accumulate, VT *vals,
                      const int *vmap_t, VT *vals_t)
{
    const SmSide<VT> a = sm_row_side<VT>(A), b = transpose_b ? sm_row_side<VT>(B) : sm_col_side<VT>(B);
    const long long nt = S->ntiles;
    if (sm_lanes_per_tile() == 64) {
        const size_t blocks = std::min(((size_t)nt + 3) / 4, kSmMaxBlocks);
        PEM_LAUNCH_NAMED(ctx, kSmNames[sizeof(VT) == 8][K][0], (sampled_kernel<VT, K, 64>), (unsigned)std::max<size_t>(blocks, 1), 256,
                         S->tile_keys.as<long long>(), S->tile_nnz_ptr.as<int>(), S->rowcolidx.as<uint8_t>(), nt, a, b, accumulate, vals, vmap_t,
                         vals_t);
    } else {
        const size_t blocks = std::min(((size_t)nt + 15) / 16, kSmMaxBlocks);
        PEM_LAUNCH_NAMED(ctx, kSmNames[sizeof(VT) == 8][K][1], (sampled_kernel<VT, K, 16>), (unsigned)std::max<size_t>(blocks, 1), 256,
                         S->tile_keys.as<long long>(), S->tile_nnz_ptr.as<int>(), S->rowcolidx.as<uint8_t>(), nt, a, b, accumulate, vals, vmap_t,
                         vals_t);
    }
}

template <typename VT>
static void sm_run(pem_ctx *ctx, const pem_tiled *S, const pem_tiled *A, const pem_tiled *B, int transpose_b, int semiring, int accumulate,
                   void *vals, const int *vmap_t, void *vals_t)
{
    VT *v = static_cast<VT *>(vals), *vt = static_cast<VT *>(vals_t);
    switch (semiring) {
    case 0: return sm_launch<VT, 0>(ctx, S, A, B, transpose_b, accumulate, v, vmap_t, vt);
    case 1: return sm_launch<VT, 1>(ctx, S, A, B, transpose_b, accumulate, v, vmap_t, vt);
    case 2: return sm_launch<VT, 2>(ctx, S, A, B, transpose_b, accumulate, v, vmap_t, vt);
    case 3: return sm_launch<VT, 3>(ctx, S, A, B, transpose_b, accumulate, v, vmap_t, vt);
    case 4: return sm_launch<VT, 4>(ctx, S, A, B, transpose_b, accumulate, v, vmap_t, vt);
    default: return sm_launch<VT, 5>(ctx, S, A, B, transpose_b, accumulate, v, vmap_t, vt);
    }
}

// the checks both entry points share (the handles are not null); nothing here touches the device
static pem_status sm_check(const pem_tiled *S, const pem_tiled *A, const pem_tiled *B, int transpose_b, int semiring, const char *fn)
{
    if (semiring < PEM_SEMIRING_PLUS_TIMES || semiring > PEM_SEMIRING_LOR_LAND) {
        set_error("%s: unknown semiring %d (PEM_SEMIRING_PLUS_TIMES .. PEM_SEMIRING_LOR_LAND = 0 .. 5)", fn, semiring);
        return PEM_E_INVALID;
    }
    if (transpose_b != 0 && transpose_b != 1) {
        set_error("%s: transpose_b must be 0 or 1 (got %d)", fn, transpose_b);
        return PEM_E_INVALID;
    }
    if (A->value_bytes != B->value_bytes) {
        set_error("%s: A holds %s values and B %s", fn, A->value_bytes == 4 ? "fp32" : "fp64", B->value_bytes == 4 ? "fp32" : "fp64");
        return PEM_E_INVALID;
    }
    const int b_inner = transpose_b ? B->cols : B->rows, b_outer = transpose_b ? B->rows : B->cols;
    if (A->cols != b_inner) {
        set_error("%s: the inner dimensions differ: A is %d x %d, B%s is %d x %d", fn, A->rows, A->cols, transpose_b ? "^T" : "", b_inner, b_outer);
        return PEM_E_INVALID;
    }
    if (S->rows != A->rows || S->cols != b_outer) {
        set_error("%s: the pattern is %d x %d, the product %d x %d", fn, S->rows, S->cols, A->rows, b_outer);
        return PEM_E_INVALID;
    }
    return PEM_OK;
}

// S's sorted tile payload copied, the values computed on S's structure into T's vals, everything else derived (as sddmm_build)
static pem_status sampled_build(pem_ctx *ctx, const pem_tiled *S, const pem_tiled *A, const pem_tiled *B, int transpose_b, int semiring,
                                pem_tiled *T)
{
    hipStream_t st = ctx->stream;
    const size_t nnz = (size_t)S->nnz, nt = (size_t)S->ntiles;
    PEM_TRY(zero_flags(ctx));
    set_tiled_shape(T, A->value_bytes, S->rows, S->cols);
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
        if (A->value_bytes == 4)
            sm_run<float>(ctx, S, A, B, transpose_b, semiring, 0, T->vals.p, nullptr, nullptr);
        else
            sm_run<double>(ctx, S, A, B, transpose_b, semiring, 0, T->vals.p, nullptr, nullptr);
    }
    PEM_TRY(derive_tiled(ctx, T, headx, bits_tr, bits_tc));
    int hf[NUM_FLAGS];
    PEM_TRY(read_flags(ctx, hf));
    return check_internal(hf);
}

extern "C" pem_status pem_tiled_sampled_mxm(pem_ctx *ctx, const pem_tiled *S, const pem_tiled *A, const pem_tiled *B, int transpose_b,
                                            int semiring, pem_tiled **out)
{
    const char *fn = "pem_tiled_sampled_mxm";
    if (out) *out = nullptr;
    if (!ctx || !S || !A || !B || !out) {
        set_error("%s: null context, tiling or output", fn);
        return PEM_E_INVALID;
    }
    PEM_TRY(sm_check(S, A, B, transpose_b, semiring, fn));
    return build_derived(ctx, out, [&](pem_tiled *T) { return sampled_build(ctx, S, A, B, transpose_b, semiring, T); });
}

extern "C" pem_status pem_tiled_set_values_sampled_mxm(pem_ctx *ctx, pem_tiled *t, const pem_tiled *A, const pem_tiled *B, int transpose_b,
                                                       int semiring, int accumulate)
{
    const char *fn = "pem_tiled_set_values_sampled_mxm";
    if (!ctx || !t || !A || !B) {
        set_error("%s: null context or tiling", fn);
        return PEM_E_INVALID;
    }
    if (accumulate != 0 && accumulate != 1) {
        set_error("%s: accumulate must be 0 or 1 (got %d)", fn, accumulate);
        return PEM_E_INVALID;
    }
    PEM_TRY(sm_check(t, A, B, transpose_b, semiring, fn));
    if (t->value_bytes != A->value_bytes) {
        set_error("%s: the tiling holds %s values, the operands %s", fn, t->value_bytes == 4 ? "fp32" : "fp64",
                  A->value_bytes == 4 ? "fp32" : "fp64");
        return PEM_E_INVALID;
    }
    if (t == A || t == B) {
        set_error("%s: the tiling is also %s: the refresh would read the values it writes", fn, t == A ? "A" : "B");
        return PEM_E_INVALID;
    }
    if (t->nnz) {
        PEM_ENTER(ctx);
        PEM_TRY(ensure_vmap_t(ctx, t));
        if (t->value_bytes == 4)
            sm_run<float>(ctx, t, A, B, transpose_b, semiring, accumulate, t->vals.p, t->vmap_t.as<int>(), t->vals_t.p);
        else
            sm_run<double>(ctx, t, A, B, transpose_b, semiring, accumulate, t->vals.p, t->vmap_t.as<int>(), t->vals_t.p);
    }
    ++t->value_version;
    return PEM_OK;
}
