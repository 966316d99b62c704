// mx_internal.h -- what the line walks over a tiling's rows or columns share (mxv.hip, spmm.hip, sddmm.hip, frontier.hip, argmxv.hip, trsv.hip; graph_internal.h, the one walk of colour.hip, components.hip and aggregate.hip; the wave sync also ilu0.hip):
// the folds of the matrix-vector products and reductions, the wave sync around the staging area, the column-walk schedule, the
// frontier's pack and mark, and the span of a dense row-major block.  SpMM folds with the
// very functions mxv folds with, so column c of A (+).(x) X is bit for bit mxv of X's column c; SDDMM folds its chains with them too.
#pragma once
#include "spgemm_internal.h"

namespace pem {

// ------------------------------------------------------------------------------------------
// the folds: K < 6 is a pem_semiring (mxv, spmm), K = 6 + op a pem_binop (reduce)
// ------------------------------------------------------------------------------------------
enum { MX_REDUCE = 6, MX_KINDS = 12 };

template <int K>
struct MxOp {
    static constexpr bool reads_vals = K != PEM_SEMIRING_PLUS_PAIR;
    static constexpr bool reads_x = K < MX_REDUCE && K != PEM_SEMIRING_PLUS_PAIR;
    static constexpr bool pair = K == PEM_SEMIRING_PLUS_TIMES;   // stages (a, x): the fma needs both unrounded
    template <typename VT> static __device__ __forceinline__ VT start()
    {
        switch (K) {
        case PEM_SEMIRING_MIN_PLUS:
        case MX_REDUCE + PEM_BINOP_MIN: return pem_inf<VT>();
        case PEM_SEMIRING_MAX_PLUS:
        case PEM_SEMIRING_MAX_TIMES:
        case MX_REDUCE + PEM_BINOP_MAX: return -pem_inf<VT>();
        case MX_REDUCE + PEM_BINOP_TIMES:
        case MX_REDUCE + PEM_BINOP_LAND: return VT(1);
        default: return VT(0);
        }
    }
    // the start taken from the old y (accumulate): the boolean folds start from y != 0
    template <typename VT> static __device__ __forceinline__ VT from_y(VT y)
    {
        if constexpr (K == PEM_SEMIRING_LOR_LAND || K == MX_REDUCE + PEM_BINOP_LOR || K == MX_REDUCE + PEM_BINOP_LAND)
            return y != VT(0) ? VT(1) : VT(0);
        else
            return y;
    }
    // what one entry contributes (every + and * rounded once in VT; -ffp-contract=off)
    template <typename VT> static __device__ __forceinline__ VT term(VT a, VT x)
    {
        switch (K) {
        case PEM_SEMIRING_MIN_PLUS:
        case PEM_SEMIRING_MAX_PLUS: return a + x;
        case PEM_SEMIRING_MAX_TIMES: return a * x;
        case PEM_SEMIRING_LOR_LAND: return (a != VT(0) && x != VT(0)) ? VT(1) : VT(0);
        default: return a;   // plus_times stages a and x apart; plus_pair's term is not read
        }
    }
    template <typename VT> static __device__ __forceinline__ VT step(VT acc, VT t, VT x)
    {
        switch (K) {
        case PEM_SEMIRING_PLUS_TIMES: return pem_fma(t, x, acc);
        case PEM_SEMIRING_MIN_PLUS:
        case MX_REDUCE + PEM_BINOP_MIN: return pem_fmin(acc, t);
        case PEM_SEMIRING_MAX_PLUS:
        case PEM_SEMIRING_MAX_TIMES:
        case MX_REDUCE + PEM_BINOP_MAX: return pem_fmax(acc, t);
        case PEM_SEMIRING_PLUS_PAIR: return acc + VT(1);
        case PEM_SEMIRING_LOR_LAND: return t != VT(0) ? VT(1) : acc;
        case MX_REDUCE + PEM_BINOP_PLUS: return acc + t;
        case MX_REDUCE + PEM_BINOP_TIMES: return acc * t;
        case MX_REDUCE + PEM_BINOP_LOR: return (acc != VT(0) || t != VT(0)) ? VT(1) : VT(0);
        default: return (acc != VT(0) && t != VT(0)) ? VT(1) : VT(0);   // reduce LAND
        }
    }
};

// the wave-level fence around a wave's own LDS staging area: what the lanes stored before it is visible to every lane after it
__device__ __forceinline__ void mx_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The column walk's schedule, built on the first column-orientation call and kept with the tiling (mxv.hip): per CSC position the
// entry offset in column-walk order (mx_csc_off) and the tile's first slot in vals_t (mx_csc_base), per vals_t slot the entry's
// (c << 4) | r (mx_rci_t).  Allocates from the context's arena the first time only; stream-ordered.
pem_status ensure_mx_cols(pem_ctx *ctx, const pem_tiled *A);

// pem_tiled_mxv's launch for checked arguments (mxv.hip): y = A (+).(x) x under semiring K < 6, col the orientation; x and y hold
// the tiling's value type.  Builds the column schedule on first use; stream-ordered.
pem_status mxv_semiring(pem_ctx *ctx, const pem_tiled *A, int semiring, bool col, const float *x, float *y, int accumulate);
pem_status mxv_semiring(pem_ctx *ctx, const pem_tiled *A, int semiring, bool col, const double *x, double *y, int accumulate);

// The frontier's pack and mark for checked arguments (frontier.hip): with an xpres, the presence word of every 16-entry segment of
// x and the flag of every line a present x can reach, in the context's grow-only scratch; without one both come back null (the
// walk's ALLX variant reads neither).  Builds the column schedule for col; records the call for pem_test_frontier_line_flags.
// Stream-ordered.  The caller has returned already where the orientation has no line.
pem_status fr_prepare(pem_ctx *ctx, const pem_tiled *A, bool col, const uint8_t *xpres, const uint16_t **words, const uint8_t **flags);

// the argument checks the frontier calls share
inline bool fr_flag_ok(int v) { return v == 0 || v == 1; }

struct Span {
    const char *lo, *hi;
    Span(const void *p, size_t bytes) : lo((const char *)p), hi((const char *)p + (p ? bytes : 0)) {}
    bool meets(const Span &o) const { return lo < hi && o.lo < o.hi && lo < o.hi && o.lo < hi; }
};

// the bytes [lo, hi) a row-major n x k block with row stride ld spans (empty when n or k is 0); false when n * ld overflows int64
// (the argument checks of spmm.hip and sddmm.hip)
inline bool sp_span(const void *p, int64_t n, int64_t k, int64_t ld, int vb, unsigned __int128 *lo, unsigned __int128 *hi)
{
    int64_t nld = 0;
    if (__builtin_mul_overflow(n, ld, &nld)) return false;
    *lo = *hi = (unsigned __int128)(uintptr_t)p;
    if (n > 0 && k > 0) *hi += ((unsigned __int128)(n - 1) * (unsigned __int128)ld + (unsigned __int128)k) * (unsigned)vb;
    return true;
}

}  // namespace pem
