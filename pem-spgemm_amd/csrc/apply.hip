// apply.hip -- new values on an unchanged pattern (include/pem_spgemm.h, pem_tiled_apply / pem_tiled_scale and their refreshes):
// R = f(A) entry by entry, and R = op(op(r_i, a_ij), c_j) with a row and a column vector.
//
// R stores exactly the positions A stores, so nothing is sorted, scanned or decoded: R's structural arrays are device copies of A's
// (clone_structure: everything derive_tiled would have produced, h_tile_rowptr included) and only vals and vals_t are computed.
//   apply   needs no coordinates.  One flat launch over both value arrays (blockIdx.y = 0: vals, 1: vals_t), four entries per lane
//           with 16- or 32-byte loads and stores and a scalar tail, so slot e of R's vals / vals_t is f of slot e of A's.  The op is
//           wave-uniform: one switch per lane and group of four, nothing per entry but the arithmetic.
//   scale   needs (i, j) per entry.  sel_value_kernel's shape: one wave per chunk of 64 consecutive tiles, one ENTRY per lane; the
//           entry's tile by chunk_tile_of, its tile row and column from the tile's key (kept in the tile's lane, fetched by a
//           shuffle), its in-tile row and column from rowcolidx.  z is computed once, stored to vals[e] (coalesced) and to
//           vals_t[vmap_t[e]], a scatter inside the tile's window of at most 2 KiB.  The 16 r values of a tile row and the 16 c
//           values of a tile column are shared by the whole tile and come from L2.  r and c are read at indices of stored entries
//           only, so a ragged last tile never reads past rows - 1 or cols - 1.
// Refreshes: the same kernels from A's arrays into t's.  apply's allocates nothing, ever; scale's needs t's vmap_t, which the build
// already made, so it allocates nothing either.  No atomics anywhere: two calls give identical bits.
//
// Arithmetic: everything in the value type, one rounding per operation (-ffp-contract=off, no fma).  x / y, 1 / x and sqrt are the
// compiler's IEEE forms: correctly rounded in fp64 and, with hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt and the
// gfx9 default of kept fp32 subnormals, in fp32 (tests/test_gpu_apply.py compares them with numpy bit for bit).
#include "spgemm_internal.h"
#include "tiled_internal.h"
#include <climits>
#include <cmath>

using namespace pem;

// ------------------------------------------------------------------------------------------
// the value rules (header comments of pem_tiled_apply and pem_tiled_scale)
// ------------------------------------------------------------------------------------------
template <typename VT>
__device__ __forceinline__ VT ap_abs(VT x)   // the sign bit cleared: a NaN keeps its payload
{
    if constexpr (sizeof(VT) == 8)
        return __longlong_as_double(__double_as_longlong(x) & 0x7FFFFFFFFFFFFFFFll);
    else
        return __uint_as_float(__float_as_uint(x) & 0x7FFFFFFFu);
}

template <typename VT>
__device__ __forceinline__ VT ap_neg(VT x)   // the sign bit flipped
{
    if constexpr (sizeof(VT) == 8)
        return __longlong_as_double(__double_as_longlong(x) ^ (long long)0x8000000000000000ull);
    else
        return __uint_as_float(__float_as_uint(x) ^ 0x80000000u);
}

template <typename VT>
__device__ __forceinline__ VT ap_sqrt(VT x)
{
    if constexpr (sizeof(VT) == 8)
        return __builtin_sqrt(x);
    else
        return __builtin_sqrtf(x);
}

// x^k by the square-and-multiply chain over the bits of k below its leading one, every product rounded once; k = 1 returns x
template <typename VT>
__device__ __forceinline__ VT ap_powi(VT x, int k)
{
    VT p = x;
    for (int b = 30 - __builtin_clz(k); b >= 0; --b) {   // (k >= 1; wave-uniform trip count)
        p = p * p;
        if ((k >> b) & 1) p = p * x;
    }
    return p;
}

// y = the thunk in the value type, k = the thunk of POWI
template <typename VT>
__device__ __forceinline__ VT ap_value(int op, VT x, VT y, int k)
{
    switch (op) {
    case PEM_APPLY_IDENTITY: return x;
    case PEM_APPLY_ABS: return ap_abs(x);
    case PEM_APPLY_AINV: return ap_neg(x);
    case PEM_APPLY_MINV: return VT(1) / x;
    case PEM_APPLY_SQRT: return ap_sqrt(x);
    case PEM_APPLY_ONE: return VT(1);
    case PEM_APPLY_PLUS: return x + y;
    case PEM_APPLY_TIMES: return x * y;
    case PEM_APPLY_MIN: return pem_fmin(x, y);
    case PEM_APPLY_MAX: return pem_fmax(x, y);
    case PEM_APPLY_DIV: return x / y;
    case PEM_APPLY_RDIV: return y / x;
    case PEM_APPLY_RMINUS: return y - x;
    default: return ap_powi(x, k);   // PEM_APPLY_POWI
    }
}

// ------------------------------------------------------------------------------------------
// apply: dst[e] = f(src[e]) over vals (blockIdx.y = 0) and vals_t (1), four entries per lane.  Both arrays start 256-byte aligned
// (arena blocks); the last nnz & 3 entries go one by one, so nothing past slot nnz - 1 is read or written.  ONE reads no values.
// ------------------------------------------------------------------------------------------
template <typename VT>
__global__ void __launch_bounds__(256) apply_kernel(const VT *__restrict__ a_vals, const VT *__restrict__ a_vals_t, size_t nnz, int op, VT y, int k,
                                                    VT *__restrict__ vals, VT *__restrict__ vals_t)
{
    const VT *__restrict__ src = blockIdx.y ? a_vals_t : a_vals;
    VT *__restrict__ dst = blockIdx.y ? vals_t : vals;
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t e = 4 * q;
    if (e >= nnz) return;
    if (e + 4 <= nnz) {
        VT v0 = VT(0), v1 = VT(0), v2 = VT(0), v3 = VT(0);
        if (op != PEM_APPLY_ONE) {
            if constexpr (sizeof(VT) == 8) {
                const double2 *p = reinterpret_cast<const double2 *>(src + e);
                const double2 lo = p[0], hi = p[1];
                v0 = lo.x, v1 = lo.y, v2 = hi.x, v3 = hi.y;
            } else {
                const float4 f = reinterpret_cast<const float4 *>(src + e)[0];
                v0 = f.x, v1 = f.y, v2 = f.z, v3 = f.w;
            }
        }
        v0 = ap_value<VT>(op, v0, y, k);
        v1 = ap_value<VT>(op, v1, y, k);
        v2 = ap_value<VT>(op, v2, y, k);
        v3 = ap_value<VT>(op, v3, y, k);
        if constexpr (sizeof(VT) == 8) {
            double2 *o = reinterpret_cast<double2 *>(dst + e);
            o[0] = make_double2(v0, v1);
            o[1] = make_double2(v2, v3);
        } else {
            reinterpret_cast<float4 *>(dst + e)[0] = make_float4(v0, v1, v2, v3);
        }
    } else {
        for (size_t i = e; i < nnz; ++i) dst[i] = ap_value<VT>(op, op != PEM_APPLY_ONE ? src[i] : VT(0), y, k);
    }
}

// ------------------------------------------------------------------------------------------
// scale: one wave per chunk of 64 consecutive tiles, one entry per lane.  Lane = tile first: its entry offset, tile row and tile
// column stay in the lane's registers.  Then every lane takes one entry of the chunk: its tile by the shuffle search, (i, j) =
// (16 tile row + r, 16 tile column + c) -- both below 2^31 by the conversion's limits on rows and cols -- and
// z = op(op(d_row[i], a), d_col[j]), a null vector's step left out.  Entry slots are 64-bit until compared with the chunk's end.
// ------------------------------------------------------------------------------------------
template <typename VT>
__global__ void __launch_bounds__(256) scale_kernel(const long long *__restrict__ keys, const int *__restrict__ ptr, const uint8_t *__restrict__ rci,
                                                    const VT *__restrict__ a_vals, long long nt, int op, const VT *__restrict__ d_row,
                                                    const VT *__restrict__ d_col, const int *__restrict__ map_t, VT *__restrict__ vals,
                                                    VT *__restrict__ vals_t)
{
    const int lane = threadIdx.x & 63;
    const long long t0 = (((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6) << 6;
    if (t0 >= nt) return;   // (wave-uniform)
    const int ntl = nt - t0 < 64 ? (int)(nt - t0) : 64;
    const bool live = lane < ntl;
    const long long o = t0 + (live ? lane : 0);
    const int my_off = live ? ptr[o] : INT_MAX;
    const int e_end = ptr[t0 + ntl];
    const long long key = keys[o];
    const int my_tr = (int)(key >> 32), my_tc = (int)(key & 0xFFFFFFFFll);
    const int e_begin = __shfl(my_off, 0, 64);
    for (long long ebase = e_begin; ebase < e_end; ebase += 64) {   // wave-uniform trip count
        const long long el = ebase + lane;
        const int e = el < e_end ? (int)el : e_end - 1;
        const int ti = chunk_tile_of(my_off, e);
        const int tr = __shfl(my_tr, ti, 64), tc = __shfl(my_tc, ti, 64);
        if (el >= e_end) continue;
        const unsigned rc = rci[e];
        VT z = a_vals[e];
        if (d_row) z = pem_binop_value<VT>(op, d_row[16 * tr + (int)(rc >> 4)], z);
        if (d_col) z = pem_binop_value<VT>(op, z, d_col[16 * tc + (int)(rc & 15u)]);
        vals[e] = z;
        vals_t[map_t[e]] = z;
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
// R's shape, sizes and structural arrays from A: device copies of everything derive_tiled produces but the values, the host copy
// of the tile row pointers too.  R's vals and vals_t are allocated and left for the caller's kernel.  One sizing phase over R's own
// arrays (and its vmap_t where the caller will fill it): none of the context's conversion scratch is needed, so none is grown.
pem_status pem::clone_structure(pem_ctx *ctx, const pem_tiled *A, pem_tiled *R, bool with_vmap_t)
{
    set_tiled_shape(R, A->value_bytes, A->rows, A->cols);
    R->nnz = A->nnz;
    R->ntiles = A->ntiles;
    const size_t nnz = (size_t)A->nnz, nt = (size_t)A->ntiles, mt = (size_t)A->tile_rows, nc = (size_t)A->tile_cols;
    const size_t vbytes = (size_t)R->value_bytes * (nnz + 1);
    struct Copy {
        DevBuf pem_tiled::*buf;
        size_t cap, bytes;   // what derive_tiled / reserve_payload reserve; what holds data
    };
    const Copy copies[] = {
        {&pem_tiled::tile_keys, 8 * (nt + 1), 8 * nt},       {&pem_tiled::tile_nnz_ptr, 4 * (nt + 4), 4 * (nt + 1)},
        {&pem_tiled::masks, 32 * (nt + 1), 32 * nt},         {&pem_tiled::masks_t, 32 * (nt + 1), 32 * nt},
        {&pem_tiled::rowptr, 16 * (nt + 1), 16 * nt},        {&pem_tiled::rowcolidx, nnz + 16, nnz},
        {&pem_tiled::tile_rec, 64 * (nt + 1), 64 * nt},      {&pem_tiled::tile_rec_t, 64 * (nt + 1), 64 * nt},
        {&pem_tiled::tile_occ, 4 * (nt + 4), 4 * nt},        {&pem_tiled::tile_colocc, 8 * (nt + 4), 8 * nt},
        {&pem_tiled::tile_rowptr, 4 * (mt + 4), 4 * (mt + 1)}, {&pem_tiled::tile_colidx, 4 * (nt + 4), 4 * nt},
        {&pem_tiled::tile_colptr, 4 * (nc + 4), 4 * (nc + 1)}, {&pem_tiled::tile_rowidx, 4 * (nt + 4), 4 * nt},
        {&pem_tiled::tile_offsets, 4 * (nt + 4), 4 * nt},
    };
    PEM_TRY(arena_phase(ctx->arena, {{&R->tile_keys, copies[0].cap},    {&R->tile_nnz_ptr, copies[1].cap}, {&R->masks, copies[2].cap},
                                     {&R->masks_t, copies[3].cap},      {&R->rowptr, copies[4].cap},       {&R->rowcolidx, copies[5].cap},
                                     {&R->tile_rec, copies[6].cap},     {&R->tile_rec_t, copies[7].cap},   {&R->tile_occ, copies[8].cap},
                                     {&R->tile_colocc, copies[9].cap},  {&R->tile_rowptr, copies[10].cap}, {&R->tile_colidx, copies[11].cap},
                                     {&R->tile_colptr, copies[12].cap}, {&R->tile_rowidx, copies[13].cap}, {&R->tile_offsets, copies[14].cap},
                                     {&R->vals, vbytes},                {&R->vals_t, vbytes},
                                     {&R->vmap_t, with_vmap_t && nnz ? sizeof(int) * (nnz + 4) : 0}}));
    PEM_TRY(R->vals.reserve(vbytes));
    PEM_TRY(R->vals_t.reserve(vbytes));
    for (const Copy &c : copies) {
        PEM_TRY((R->*c.buf).reserve(c.cap));
        if (c.bytes) PEM_HIP(hipMemcpyAsync((R->*c.buf).p, (A->*c.buf).p, c.bytes, hipMemcpyDeviceToDevice, ctx->stream));
    }
    R->h_tile_rowptr = A->h_tile_rowptr;
    return PEM_OK;
}

// the tail of both builds: the value kernels ran between ev[6] and here
static pem_status finish_build(pem_ctx *ctx, pem_tiled *R)
{
    PEM_HIP(hipEventRecord(ctx->ev[7], ctx->stream));
    PEM_HIP(hipStreamSynchronize(ctx->stream));
    PEM_TRY(launch_status(ctx));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ctx->ev[6], ctx->ev[7]) == hipSuccess) R->conv_tile_kernel_ms = ms;
    return PEM_OK;
}

template <typename VT>
static void launch_apply(pem_ctx *ctx, const pem_tiled *A, pem_tiled *R, int op, double thunk)
{
    const size_t nnz = (size_t)A->nnz;
    if (!nnz) return;
    PEM_LAUNCH_NAMED(ctx, sizeof(VT) == 4 ? "apply_kernel<float>" : "apply_kernel<double>", apply_kernel<VT>, dim3(grid_for((nnz + 3) / 4, 256), 2), 256,
                     A->vals.as<VT>(), A->vals_t.as<VT>(), nnz, op, (VT)thunk, op == PEM_APPLY_POWI ? (int)thunk : 1, R->vals.as<VT>(),
                     R->vals_t.as<VT>());
}

// R's vmap_t must be ready
template <typename VT>
static void launch_scale(pem_ctx *ctx, const pem_tiled *A, pem_tiled *R, int op, const void *d_row, const void *d_col)
{
    const size_t nt = (size_t)A->ntiles;
    if (!A->nnz) return;
    PEM_LAUNCH_NAMED(ctx, sizeof(VT) == 4 ? "scale_kernel<float>" : "scale_kernel<double>", scale_kernel<VT>, grid_for((nt + 63) / 64 * 64, 256), 256,
                     A->tile_keys.as<long long>(), A->tile_nnz_ptr.as<int>(), A->rowcolidx.as<uint8_t>(), A->vals.as<VT>(), (long long)nt, op,
                     static_cast<const VT *>(d_row), static_cast<const VT *>(d_col), R->vmap_t.as<int>(), R->vals.as<VT>(), R->vals_t.as<VT>());
}

static bool apply_args_ok(int op, double thunk, const char *fn)
{
    if (op < PEM_APPLY_IDENTITY || op > PEM_APPLY_POWI) {
        set_error("%s: unknown op %d (PEM_APPLY_IDENTITY .. PEM_APPLY_POWI = 0 .. 13)", fn, op);
        return false;
    }
    if (op == PEM_APPLY_POWI && !(std::floor(thunk) == thunk && thunk >= 1.0 && thunk <= 64.0)) {
        set_error("%s: the thunk of PEM_APPLY_POWI must be an integer k in 1 .. 64, not %g", fn, thunk);
        return false;
    }
    return true;
}

extern "C" pem_status pem_tiled_apply(pem_ctx *ctx, const pem_tiled *A, int op, double thunk, pem_tiled **out)
{
    const char *fn = "pem_tiled_apply";
    if (out) *out = nullptr;
    if (!ctx || !A || !out) {
        set_error("%s: null context, operand or output", fn);
        return PEM_E_INVALID;
    }
    if (!apply_args_ok(op, thunk, fn)) return PEM_E_INVALID;
    return build_derived(ctx, out, [&](pem_tiled *R) -> pem_status {
        R->derived.kind = Derivation::APPLY;
        R->derived.src[0] = A->serial;
        R->derived.op = op;
        R->derived.p0 = thunk;
        PEM_TRY(clone_structure(ctx, A, R, false));
        PEM_HIP(hipEventRecord(ctx->ev[6], ctx->stream));
        if (A->value_bytes == 4)
            launch_apply<float>(ctx, A, R, op, thunk);
        else
            launch_apply<double>(ctx, A, R, op, thunk);
        return finish_build(ctx, R);
    });
}

extern "C" pem_status pem_tiled_set_values_from_apply(pem_ctx *ctx, pem_tiled *t, const pem_tiled *A)
{
    const char *fn = "pem_tiled_set_values_from_apply";
    if (!ctx || !t || !A) {
        set_error("%s: null context, tiling or source", fn);
        return PEM_E_INVALID;
    }
    if (t->derived.kind != Derivation::APPLY || t->derived.src[0] != A->serial) {
        set_error("%s: the tiling was not made by pem_tiled_apply from this A", fn);
        return PEM_E_INVALID;
    }
    // (refresh_derived's body without its ensure_vmap_t: slot e is computed from slot e, so this refresh needs no map and must
    // allocate nothing, not even on its first call)
    if (t->nnz) {
        PEM_ENTER(ctx);
        if (t->value_bytes == 4)
            launch_apply<float>(ctx, A, t, t->derived.op, t->derived.p0);
        else
            launch_apply<double>(ctx, A, t, t->derived.op, t->derived.p0);
    }
    ++t->value_version;
    return PEM_OK;
}

static pem_status scale_build(pem_ctx *ctx, const pem_tiled *A, int op, const void *d_row, const void *d_col, int value_bytes, pem_tiled **out,
                              const char *fn)
{
    if (out) *out = nullptr;
    if (!ctx || !A || !out) {
        set_error("%s: null context, operand or output", fn);
        return PEM_E_INVALID;
    }
    if (op < PEM_BINOP_PLUS || op > PEM_BINOP_LAND) {
        set_error("%s: unknown op %d (a pem_binop: PEM_BINOP_PLUS .. PEM_BINOP_LAND = 0 .. 5)", fn, op);
        return PEM_E_INVALID;
    }
    if (A->value_bytes != value_bytes) {
        set_error("%s: the tiling holds %s values; use the %s entry point", fn, A->value_bytes == 4 ? "fp32" : "fp64", A->value_bytes == 4 ? "_f32" : "fp64");
        return PEM_E_INVALID;
    }
    return build_derived(ctx, out, [&](pem_tiled *R) -> pem_status {
        R->derived.kind = Derivation::SCALE;
        R->derived.src[0] = A->serial;
        R->derived.op = op;
        PEM_TRY(clone_structure(ctx, A, R, true));
        if (R->nnz) PEM_TRY(ensure_vmap_t(ctx, R));
        PEM_HIP(hipEventRecord(ctx->ev[6], ctx->stream));
        if (value_bytes == 4)
            launch_scale<float>(ctx, A, R, op, d_row, d_col);
        else
            launch_scale<double>(ctx, A, R, op, d_row, d_col);
        return finish_build(ctx, R);
    });
}

static pem_status scale_refresh(pem_ctx *ctx, pem_tiled *t, const pem_tiled *A, const void *d_row, const void *d_col, int value_bytes, const char *fn)
{
    if (!ctx || !t || !A) {
        set_error("%s: null context, tiling or source", fn);
        return PEM_E_INVALID;
    }
    if (t->derived.kind != Derivation::SCALE || t->derived.src[0] != A->serial) {
        set_error("%s: the tiling was not made by pem_tiled_scale from this A", fn);
        return PEM_E_INVALID;
    }
    if (t->value_bytes != value_bytes) {
        set_error("%s: the tiling holds %s values; use the %s entry point", fn, t->value_bytes == 4 ? "fp32" : "fp64", t->value_bytes == 4 ? "_f32" : "fp64");
        return PEM_E_INVALID;
    }
    return refresh_derived(
        ctx, t, [] { return PEM_OK; },
        [&] {
            if (value_bytes == 4)
                launch_scale<float>(ctx, A, t, t->derived.op, d_row, d_col);
            else
                launch_scale<double>(ctx, A, t, t->derived.op, d_row, d_col);
        });
}

extern "C" pem_status pem_tiled_scale(pem_ctx *ctx, const pem_tiled *A, int op, const double *d_row, const double *d_col, pem_tiled **out)
{
    return scale_build(ctx, A, op, d_row, d_col, 8, out, "pem_tiled_scale");
}
extern "C" pem_status pem_tiled_scale_f32(pem_ctx *ctx, const pem_tiled *A, int op, const float *d_row, const float *d_col, pem_tiled **out)
{
    return scale_build(ctx, A, op, d_row, d_col, 4, out, "pem_tiled_scale_f32");
}
extern "C" pem_status pem_tiled_set_values_from_scale(pem_ctx *ctx, pem_tiled *t, const pem_tiled *A, const double *d_row, const double *d_col)
{
    return scale_refresh(ctx, t, A, d_row, d_col, 8, "pem_tiled_set_values_from_scale");
}
extern "C" pem_status pem_tiled_set_values_from_scale_f32(pem_ctx *ctx, pem_tiled *t, const pem_tiled *A, const float *d_row, const float *d_col)
{
    return scale_refresh(ctx, t, A, d_row, d_col, 4, "pem_tiled_set_values_from_scale_f32");
}
