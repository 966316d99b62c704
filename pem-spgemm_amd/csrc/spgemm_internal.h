// spgemm_internal.h -- what the translation units of the three-step hot path share (step1.hip, step2.hip, step3.hip,
// export.hip, spgemm.hip): constants that tie a producer kernel to its consumer, the repeat-pass size check, the fused
// multiply-add of step 3, and the host-side step drivers.
#pragma once
#include "pem_internal.h"
#include <algorithm>
#include <chrono>

namespace pem {

constexpr int S3_CHUNK = 256;   // C entries per chunk of step 3's work index (= entries one wave takes, or half of them)
constexpr int S2_GROUP = 256;   // C tiles per group of step 2's entry counts
constexpr int S2_FOLD_GROUPS = 8192;   // ... and how many groups s2_offsets_kernel sums in front of its own (at most eight 16-byte loads per thread)

// repeat pass on an unchanged plan: the sizes the host assumed (from the previous pass) against what this pass computed
// counters of a pass of step 1 (plan->bin_count, ints): populations of the five row bins and of the oversized rows, the
// oversized rows' live products (total, largest row), and the allocator of the live list
enum { BC_BIN0 = 0, BC_XL_ROWS = 5, BC_XL_TOTAL = 6, BC_XL_MAX = 7, BC_SEGS = 8 /* segments of the big rows */, BC_FAULT = 9, BC_BUMP = 10 /* 64-bit: ints 10-11 */, BC_INTS = 16 };

struct WarmCheck {
    int on;
    long long P, Pall, TC, nnz, nxl;
    int c[5];
    int nsegs;    int *host_flags;     // where set: the pass's status flags are left in host memory by the checking thread (no copy node after the pass)
    int masked;                        // masked plan: the mask filter's kept pairs and C tiles (d_scalars[4], [5]) are compared too
    long long Pm, TCm;
};
// (nnz_now: the pass's C_nnz -- d_scalars[2], or the value itself where the checking thread is the one that computed it)
__device__ __forceinline__ void warm_check(const WarmCheck &w, const long long *__restrict__ d_scalars, const int *__restrict__ bin_count,
                                           int *__restrict__ flags, const long long nnz_now)
{
    if (d_scalars[0] != w.P || d_scalars[1] != w.TC || nnz_now != w.nnz || d_scalars[3] != w.Pall || bin_count[0] != w.c[0] ||
        bin_count[1] != w.c[1] || bin_count[2] != w.c[2] || bin_count[3] != w.c[3] || bin_count[4] != w.c[4] || bin_count[BC_XL_TOTAL] != w.nxl || bin_count[BC_SEGS] != w.nsegs)
        flags[FLAG_CAPACITY] = 1;
    if (w.masked && (d_scalars[4] != w.Pm || d_scalars[5] != w.TCm)) flags[FLAG_CAPACITY] = 1;
    if (w.host_flags) {
        // the caller guarantees that nothing after this thread sets a flag in this pass (s2_offsets_kernel + step 3: none do)
        for (int i = 0; i < NUM_FLAGS; ++i) w.host_flags[i] = flags[i];
    }
}
__device__ __forceinline__ void warm_check(const WarmCheck &w, const long long *__restrict__ d_scalars, const int *__restrict__ bin_count,
                                           int *__restrict__ flags)
{
    warm_check(w, d_scalars, bin_count, flags, d_scalars[2]);
}

// the size check of a repeat pass of this plan (host_flags unset)
inline WarmCheck warm_check_of(const pem_cplan *p)
{
    return WarmCheck{1, p->w_P, p->w_Pall, p->w_TC, p->w_nnz, p->w_nxl, {p->w_counts[0], p->w_counts[1], p->w_counts[2], p->w_counts[3], p->w_counts[4]},
                     p->w_nsegs, nullptr, p->M != nullptr, p->w_Pm, p->w_TCm};
}

// one fused multiply-add per product in the operands' own precision (the oracle's chain; the reference computes in
// double, spgemm.cu:728 -- fp32 is SURVEY 8(f)-3)
__device__ __forceinline__ double pem_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float pem_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// Step 3's reduction as a compile-time policy (include/pem_spgemm.h, pem_semiring): the accumulator's start value, how one
// product (a, b) enters it, and whether the operands' values are read at all.  A policy without values (plus_pair) adds the
// number of products a (pair, entry) meets, __popc(Amask[r] & BT[c]), through count(); the kernels then gather no value.
// SrPlusTimes is today's chain: start VT(0), one pem_fma per product.  The min/max policies round every a + b / a * b once in
// VT (-ffp-contract=off: no fma) and reduce with fmin / fmax, which skip NaN.
template <typename VT> __device__ __forceinline__ VT pem_inf() { return sizeof(VT) == 8 ? (VT)__builtin_huge_val() : (VT)__builtin_huge_valf(); }
template <typename VT> __device__ __forceinline__ VT pem_fmin(VT x, VT y) { if constexpr (sizeof(VT) == 8) return __builtin_fmin(x, y); else return __builtin_fminf(x, y); }
template <typename VT> __device__ __forceinline__ VT pem_fmax(VT x, VT y) { if constexpr (sizeof(VT) == 8) return __builtin_fmax(x, y); else return __builtin_fmaxf(x, y); }
// a pem_binop on two stored values in the value type, rounded once (pem_tiled_ewise's both-stored arithmetic at alpha = beta = 1):
// what ewise.hip, apply.hip's scale, kron.hip and build.hip's fold of duplicates compute
template <typename VT> __device__ __forceinline__ VT pem_binop_value(int op, VT a, VT b)
{
    switch (op) {
    case PEM_BINOP_PLUS: return a + b;
    case PEM_BINOP_TIMES: return a * b;
    case PEM_BINOP_MIN: return pem_fmin(a, b);
    case PEM_BINOP_MAX: return pem_fmax(a, b);
    case PEM_BINOP_LOR: return (a != VT(0) || b != VT(0)) ? VT(1) : VT(0);
    default: return (a != VT(0) && b != VT(0)) ? VT(1) : VT(0);   // PEM_BINOP_LAND
    }
}
struct SrPlusTimes {
    static constexpr bool vals = true;
    template <typename VT> static __device__ __forceinline__ VT start() { return VT(0); }
    template <typename VT> static __device__ __forceinline__ VT combine(VT a, VT b, VT acc) { return pem_fma(a, b, acc); }
};
struct SrMinPlus {
    static constexpr bool vals = true;
    template <typename VT> static __device__ __forceinline__ VT start() { return pem_inf<VT>(); }
    template <typename VT> static __device__ __forceinline__ VT combine(VT a, VT b, VT acc) { return pem_fmin(acc, a + b); }
};
struct SrMaxPlus {
    static constexpr bool vals = true;
    template <typename VT> static __device__ __forceinline__ VT start() { return -pem_inf<VT>(); }
    template <typename VT> static __device__ __forceinline__ VT combine(VT a, VT b, VT acc) { return pem_fmax(acc, a + b); }
};
struct SrMaxTimes {
    static constexpr bool vals = true;
    template <typename VT> static __device__ __forceinline__ VT start() { return -pem_inf<VT>(); }
    template <typename VT> static __device__ __forceinline__ VT combine(VT a, VT b, VT acc) { return pem_fmax(acc, a * b); }
};
struct SrPlusPair {
    static constexpr bool vals = false;
    template <typename VT> static __device__ __forceinline__ VT start() { return VT(0); }
    template <typename VT> static __device__ __forceinline__ VT combine(VT, VT, VT acc) { return acc + VT(1); }
    // the products of one (pair, entry): the bits of m
    template <typename VT> static __device__ __forceinline__ VT count(unsigned m, VT acc) { return acc + VT(__popc(m)); }
};
struct SrLorLand {
    static constexpr bool vals = true;
    template <typename VT> static __device__ __forceinline__ VT start() { return VT(0); }
    template <typename VT> static __device__ __forceinline__ VT combine(VT a, VT b, VT acc) { return (a != VT(0) && b != VT(0)) ? VT(1) : acc; }
};

// host side (each in the unit of its step)
pem_status step_elapsed(pem_ctx *ctx, int e0, int e1, double *dst);
void retire_graph(pem_ctx *ctx, pem_cplan *plan);
pem_status step1_impl(pem_ctx *ctx, pem_cplan *p, bool allow_warm);
pem_status step2_impl(pem_ctx *ctx, pem_cplan *p);
pem_status step3_impl(pem_ctx *ctx, pem_cplan *p);
// masked plans (mask.hip): step 1's lists -> those of C<M>; *P / *TC: the unmasked counts in, the kept ones out
void mask_restore_lists(pem_cplan *p);
pem_status mask_filter(pem_ctx *ctx, pem_cplan *p, int64_t *P, int64_t *TC);
pem_status ensure_compact(pem_ctx *ctx, const pem_cplan *cp);       // _C_tileColIdx / pair offsets in the reference layout
pem_status ensure_c_rowidx(pem_ctx *ctx, const pem_cplan *p);       // _C_tileRowIdx
pem_status ensure_c_rowptr(pem_ctx *ctx, const pem_cplan *p);       // Ctiles_rowPtr
pem_status ensure_c_rowcolidx(pem_ctx *ctx, const pem_cplan *cp);   // Ctiles_rowColIdx

// C's values were computed from the operands' current values: PEM_E_STATE after a numeric refresh (pem_tiled_set_values*) of
// A or B that no step 3 has followed yet
inline pem_status c_values_current(const pem_cplan *p, const char *fn)
{
    if (p->c_semiring != p->semiring) {   // ... or after pem_cplan_set_semiring
        set_error("%s: the plan's semiring was changed (pem_cplan_set_semiring) after C was computed; run pem_spgemm_step3 or pem_spgemm first", fn);
        return PEM_E_STATE;
    }
    if (p->a_version == p->A->value_version && p->b_version == p->B->value_version) return PEM_OK;
    set_error("%s: the values of %s were refreshed (pem_tiled_set_values) after C was computed; run pem_spgemm_step3 or pem_spgemm first", fn,
              p->a_version != p->A->value_version ? "A" : "B");
    return PEM_E_STATE;
}
inline void note_c_values(pem_cplan *p)   // step 3 has just completed
{
    p->a_version = p->A->value_version;
    p->b_version = p->B->value_version;
    p->c_semiring = p->semiring;
}

}  // namespace pem
