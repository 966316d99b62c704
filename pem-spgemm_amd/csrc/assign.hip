// assign.hip -- writing a submatrix back (include/pem_spgemm.h): Z = C with Z(I, J) = A or Z(I, J) = op(C(I, J), A) (pem_tiled_assign,
// pem_tiled_assign_device) and its refresh (pem_tiled_set_values_from_assign).  The dual of extract.hip's A(I, J).
//
// Z is a new tiling; the route is glue around three routes the library has, each entered through an internal argument
// (tiled_internal.h), and two kernels of its own:
//   inverse lists   inv_i[C.rows] = p where I[p] == i, else -1 (inv_j alike; a null list is the identity and has no stage).  One lane
//                   per list element: the range check (FLAG_RANGE) and atomicCAS(&inv[L[p]], -1, p); a CAS that finds another p there
//                   is a repeated index (FLAG_REPEAT).  The call is refused on either flag, so the order of the atomics never shows.
//                   A ballot over inv packs the membership words: one 16-bit word per tile row (tile column) of C, bit r = row
//                   16P + r is in I.
//   scatter         S = A(inv_i, inv_j), of C's shape: A's entries at their destinations.  extract.hip's row gather (and the two
//                   transposes for the column side) where an index of -1 is an output row without entries (scatter_tiling).
//   region drop     without an accum only: C' = C without its entries in I x J.  select.hip's positional route with the region
//                   predicate, one lane per tile on the membership words (drop_region); no per-entry work.
//   merge           Z = C' (+) S over the union of the patterns (ewise.hip, union_tiling): disjoint, so every value is copied bit
//                   for bit.  With an accum Z = op(C, S) and there is no region drop.
// Every value is written once and no atomic touches a value: two calls give identical bytes.
//
// Refresh: Z's pattern does not depend on any value.  The first call fills ewise's int2 per entry -- (slot in C's vals, slot in A's
// vals), -1: none -- by decoding every entry's (i, j): inside the region (inv_i[i] >= 0 and inv_j[j] >= 0) A's slot at (p, q), and
// C's slot too under an accum; outside it C's slot.  Every call is then ewise.hip's refresh kernel on C's and A's vals.
#include "spgemm_internal.h"
#include "tiled_internal.h"
#include <climits>
#include <vector>

using namespace pem;

// ------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------
// one lane per list element p: inv[L[p]] = p (inv was filled with -1).  A bad index is never an address.
__global__ void as_inverse_kernel(const int *__restrict__ L, long long n, int dim, int *__restrict__ inv, int *__restrict__ flags)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int i = L[p];
    if (i < 0 || i >= dim)
        flags[FLAG_RANGE] = 1;
    else if (atomicCAS(&inv[i], -1, (int)p) != -1)
        flags[FLAG_REPEAT] = 1;
}

// one lane per index i < 16 * nt: bits[P] = bit r set where inv[16P + r] >= 0 (nt = tile rows or tile columns; dim = inv's length)
__global__ void __launch_bounds__(256) as_pack_kernel(const int *__restrict__ inv, int dim, long long nt, uint16_t *__restrict__ bits)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = i < dim && inv[i] >= 0;
    const unsigned long long b = __ballot(in);   // (every lane of the wave takes part)
    if ((threadIdx.x & 15) == 0 && (i >> 4) < nt) bits[i >> 4] = (uint16_t)((b >> (16 * ((threadIdx.x & 63) >> 4))) & 0xFFFFull);
}

// the slot in T's vals of T's entry at (i, j), -1 where T stores none
__device__ __forceinline__ int as_slot(const int *__restrict__ rowptr, const int *__restrict__ colidx, const int *__restrict__ ptr,
                                       const uint32_t *__restrict__ rec, const int i, const int j)
{
    const int t = mask_find_tile(rowptr, colidx, i >> 4, j >> 4);
    if (t < 0) return -1;
    const uint32_t w = rec[16 * (size_t)t + (i & 15)];
    return (w >> (j & 15)) & 1u ? src_slot(ptr[t], w, (unsigned)(j & 15)) : -1;
}

// the refresh map, once.  Entry (i, j) of Z: inside the region A's slot at (inv_i[i], inv_j[j]) and, with an accum, C's at (i, j);
// outside it C's.
__global__ void __launch_bounds__(256) as_map_kernel(const long long *__restrict__ z_keys, long long nt, const int *__restrict__ z_ptr,
                                                     const uint8_t *__restrict__ z_rci, const int *__restrict__ inv_i,
                                                     const int *__restrict__ inv_j, int accum, const int *__restrict__ c_rowptr,
                                                     const int *__restrict__ c_colidx, const int *__restrict__ c_ptr,
                                                     const uint32_t *__restrict__ c_rec, const int *__restrict__ a_rowptr,
                                                     const int *__restrict__ a_colidx, const int *__restrict__ a_ptr,
                                                     const uint32_t *__restrict__ a_rec, int2 *__restrict__ map)
{
    for_tile_entries(z_keys, nt, z_ptr, z_rci, [&](const int e, const long long il, const long long jl) {
        const int i = (int)il, j = (int)jl;   // (below Z's rows and columns)
        const int p = inv_i ? inv_i[i] : i, q = inv_j ? inv_j[j] : j;
        const bool inside = p >= 0 && q >= 0;
        const int sa = inside ? as_slot(a_rowptr, a_colidx, a_ptr, a_rec, p, q) : -1;
        const int sc = !inside || accum ? as_slot(c_rowptr, c_colidx, c_ptr, c_rec, i, j) : -1;
        map[e] = make_int2(sc, sa);
    });
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
static bool accum_ok(int accum) { return accum == PEM_ACCUM_NONE || (accum >= PEM_BINOP_PLUS && accum <= PEM_BINOP_LAND); }

// Z from device lists (null: all).  The inverses go into Z's derivation; everything else goes back to the arena.
static pem_status assign_build(pem_ctx *ctx, const pem_tiled *C, const pem_tiled *A, const int32_t *I, int64_t ni, const int32_t *J, int64_t nj,
                               bool on_device, int accum, pem_tiled *Z, const char *fn)
{
    const int32_t *L[2] = {I, J};
    const int64_t n[2] = {ni, nj};
    const int dim[2] = {C->rows, C->cols};
    const int64_t ntile[2] = {((int64_t)C->rows + 15) / 16, ((int64_t)C->cols + 15) / 16};
    const int *inv[2] = {nullptr, nullptr};
    const uint16_t *bits[2] = {nullptr, nullptr};
    DevBuf list[2], words[2];
    PEM_TRY(zero_flags(ctx));
    for (int k = 0; k < 2; ++k) {
        if (!L[k]) continue;
        const int *dl = L[k];
        if (!on_device) {
            PEM_TRY(list[k].reserve(sizeof(int) * ((size_t)n[k] + 4)));
            PEM_HIP(hipMemcpyAsync(list[k].p, L[k], sizeof(int) * (size_t)n[k], hipMemcpyHostToDevice, ctx->stream));
            dl = list[k].as<int>();
        }
        DevBuf &b = Z->derived.idx[k];
        PEM_TRY(b.reserve(sizeof(int) * ((size_t)dim[k] + 4)));
        PEM_TRY(words[k].reserve(sizeof(uint16_t) * ((size_t)ntile[k] + 8)));
        PEM_HIP(hipMemsetAsync(b.p, 0xFF, sizeof(int) * ((size_t)dim[k] + 4), ctx->stream));
        PEM_LAUNCH(ctx, as_inverse_kernel, grid_for((size_t)n[k], 256), 256, dl, (long long)n[k], dim[k], b.as<int>(), ctx->d_flags);
        PEM_LAUNCH(ctx, as_pack_kernel, grid_for(16 * (size_t)ntile[k], 256), 256, b.as<int>(), dim[k], (long long)ntile[k], words[k].as<uint16_t>());
        inv[k] = b.as<int>();
        bits[k] = words[k].as<uint16_t>();
    }
    int hf[NUM_FLAGS];
    PEM_TRY(read_flags(ctx, hf));   // (synchronises: the lists have been read)
    if (hf[FLAG_RANGE]) {
        set_error("%s: an index is negative or not below C's dimension (C is %d x %d)", fn, C->rows, C->cols);
        return PEM_E_INVALID;
    }
    if (hf[FLAG_REPEAT]) {
        set_error("%s: a list repeats an index (assign is defined for lists without repeats only)", fn);
        return PEM_E_INVALID;
    }
    PEM_TRY(check_internal(hf));
    list[0].release();
    list[1].release();

    std::unique_ptr<pem_tiled> S, D;   // A at its destinations; C without the region
    const pem_tiled *src = A, *base = C;
    if (inv[0] || inv[1]) {
        S.reset(new pem_tiled());
        PEM_TRY(scatter_tiling(ctx, A, inv[0], C->rows, inv[1], C->cols, S.get(), fn));
        src = S.get();
    }
    if (accum == PEM_ACCUM_NONE) {
        D.reset(new pem_tiled());
        PEM_TRY(drop_region(ctx, C, bits[0], bits[1], D.get(), fn));
        base = D.get();
    }
    words[0].release();
    words[1].release();
    PEM_TRY(union_tiling(ctx, base, src, accum == PEM_ACCUM_NONE ? (int)PEM_BINOP_PLUS : accum, Z, fn));
    (void)hipStreamSynchronize(ctx->stream);   // (S and D go back to the arena)
    Derivation &d = Z->derived;   // (union_tiling left ewise's record of the two intermediates)
    d.kind = Derivation::ASSIGN;
    d.src[0] = C->serial;
    d.src[1] = A->serial;
    d.op = accum;
    d.pattern = 0;
    d.p0 = d.p1 = 0.0;
    d.src_tiles.release();
    return PEM_OK;
}

static bool list_size_ok(const void *L, int64_t n, const char *which, const char *fn)
{
    if (L && (n < 1 || n > 0x7FFFFFFFll)) {
        set_error("%s: %s has %lld indices; a list holds 1 .. INT32_MAX of them (a null list is all)", fn, which, (long long)n);
        return false;
    }
    return true;
}

// range and repeats of a host list
static bool host_list_ok(const int32_t *L, int64_t n, int dim, const char *which, const char *fn)
{
    if (!L) return true;
    std::vector<bool> seen((size_t)dim, false);
    for (int64_t k = 0; k < n; ++k) {
        if (L[k] < 0 || L[k] >= dim) {
            set_error("%s: %s[%lld] = %d is outside 0 .. %d", fn, which, (long long)k, (int)L[k], dim - 1);
            return false;
        }
        if (seen[(size_t)L[k]]) {
            set_error("%s: %s repeats the index %d (at %lld); assign is defined for lists without repeats only", fn, which, (int)L[k], (long long)k);
            return false;
        }
        seen[(size_t)L[k]] = true;
    }
    return true;
}

static pem_status assign_entry(pem_ctx *ctx, const pem_tiled *C, const pem_tiled *A, const int32_t *I, int64_t ni, const int32_t *J, int64_t nj,
                               int accum, bool on_device, pem_tiled **out, const char *fn)
{
    if (!ctx || !C || !A || !out) {
        set_error("%s: null context, operand or output", fn);
        return PEM_E_INVALID;
    }
    *out = nullptr;
    if (!accum_ok(accum)) {
        set_error("%s: unknown accum %d (PEM_ACCUM_NONE = -1 or PEM_BINOP_PLUS .. PEM_BINOP_LAND = 0 .. 5)", fn, accum);
        return PEM_E_INVALID;
    }
    if (C->value_bytes != A->value_bytes) {
        set_error("%s: C holds %s values, A %s", fn, C->value_bytes == 4 ? "fp32" : "fp64", A->value_bytes == 4 ? "fp32" : "fp64");
        return PEM_E_INVALID;
    }
    if (!list_size_ok(I, ni, "I", fn) || !list_size_ok(J, nj, "J", fn)) return PEM_E_INVALID;
    const int64_t want_r = I ? ni : C->rows, want_c = J ? nj : C->cols;
    if (A->rows != want_r || A->cols != want_c) {
        set_error("%s: A is %d x %d, the region is %lld x %lld", fn, A->rows, A->cols, (long long)want_r, (long long)want_c);
        return PEM_E_INVALID;
    }
    if (!on_device && (!host_list_ok(I, ni, C->rows, "I", fn) || !host_list_ok(J, nj, C->cols, "J", fn))) return PEM_E_INVALID;
    return build_derived(ctx, out, [&](pem_tiled *Z) {
        pem_status s = assign_build(ctx, C, A, I, ni, J, nj, on_device, accum, Z, fn);
        (void)hipStreamSynchronize(ctx->stream);   // (the intermediates went back to the arena)
        return s;
    });
}

extern "C" pem_status pem_tiled_assign(pem_ctx *ctx, const pem_tiled *C, const pem_tiled *A, const int32_t *I, int64_t ni, const int32_t *J,
                                       int64_t nj, int accum, pem_tiled **out)
{
    return assign_entry(ctx, C, A, I, ni, J, nj, accum, false, out, "pem_tiled_assign");
}

extern "C" pem_status pem_tiled_assign_device(pem_ctx *ctx, const pem_tiled *C, const pem_tiled *A, const int32_t *dI, int64_t ni, const int32_t *dJ,
                                              int64_t nj, int accum, pem_tiled **out)
{
    return assign_entry(ctx, C, A, dI, ni, dJ, nj, accum, true, out, "pem_tiled_assign_device");
}

// once: every entry's slots in C's and A's vals
static pem_status assign_map(pem_ctx *ctx, pem_tiled *t, const pem_tiled *C, const pem_tiled *A)
{
    const size_t nnz = (size_t)t->nnz, nt = (size_t)t->ntiles;
    PEM_TRY(t->derived.map.reserve(sizeof(int2) * (nnz + 1)));
    PEM_LAUNCH(ctx, as_map_kernel, grid_for((nt + 63) / 64 * 64, 256), 256, t->tile_keys.as<long long>(), (long long)nt, t->tile_nnz_ptr.as<int>(),
               t->rowcolidx.as<uint8_t>(), t->derived.idx[0].as<int>(), t->derived.idx[1].as<int>(), t->derived.op != PEM_ACCUM_NONE ? 1 : 0,
               C->tile_rowptr.as<int>(), C->tile_colidx.as<int>(), C->tile_nnz_ptr.as<int>(), C->tile_rec.as<uint32_t>(), A->tile_rowptr.as<int>(),
               A->tile_colidx.as<int>(), A->tile_nnz_ptr.as<int>(), A->tile_rec.as<uint32_t>(), t->derived.map.as<int2>());
    return PEM_OK;
}

extern "C" pem_status pem_tiled_set_values_from_assign(pem_ctx *ctx, pem_tiled *t, const pem_tiled *C, const pem_tiled *A)
{
    const char *fn = "pem_tiled_set_values_from_assign";
    if (!ctx || !t || !C || !A) {
        set_error("%s: null context, tiling or operand", fn);
        return PEM_E_INVALID;
    }
    if (t->derived.kind != Derivation::ASSIGN || t->derived.src[0] != C->serial || t->derived.src[1] != A->serial) {
        set_error("%s: the tiling was not made by pem_tiled_assign from this C and this A (in this order)", fn);
        return PEM_E_INVALID;
    }
    const int op = t->derived.op == PEM_ACCUM_NONE ? (int)PEM_BINOP_PLUS : t->derived.op;   // (without an accum no entry has both)
    return refresh_derived(
        ctx, t, [&] { return assign_map(ctx, t, C, A); }, [&] { refresh_pairs(ctx, t, C->vals.p, A->vals.p, op); });
}
