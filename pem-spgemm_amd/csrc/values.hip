// values.hip -- numeric refresh: new values written into an existing tiling in place (include/pem_spgemm.h,
// pem_tiled_set_values*).  The reference has no counterpart: its timed loop re-runs the whole pipeline.
//
// Steps 1 and 2 read only the structure of A and B, and C's structure does not depend on values, so a tiling whose values
// change keeps every plan's steps 1-2 valid: step 3 alone recomputes C.  What a refresh has to do is put the caller's
// values where the tiling keeps them, in both value layouts -- vals (tile order, row-major inside a tile) and vals_t
// (tile order, column-major inside a tile).
//
// Two int32[nnz] maps make that one gather per entry:
//   vmap[order][e] -- where entry e (tile storage order) finds its value in V.  Built on the first refresh in that order by a
//                     count, a scan and a write -- no sort.  Row-major order: the entries in front of entry (t, r, c) are those
//                     of the rows before matrix row 16R+r (R = tile row of t), those of row r in the tiles of tile row R left
//                     of t, and the ones left of c in the tile's row r.  So the row populations laid out as (tile row,
//                     local row, tile) -- slot 16 tile_rowptr[R] + r n_R + (t - tile_rowptr[R]) -- and scanned give every
//                     (tile, row) run its first position in V.  Column-major order is the same over the tile CSC and the
//                     transposed masks.
//   vmap_t[e]      -- entry e's slot in vals_t (the formula of conv_vals_t_kernel), built once per tiling.
// The refresh kernel then reads map, map_t and V and writes vals and vals_t: 32 bytes per fp64 entry against the 28 the
// copy needs.  A tile-parallel kernel (16 lanes per tile, the vals_t slot from the tile's transposed records) would save
// vmap_t's 4 bytes but read ~100 bytes of records per TILE and idle most lanes on the sparse tiles of web graphs (a few
// entries per tile); the entry-parallel kernel's traffic does not depend on how full the tiles are.
#include "spgemm_internal.h"
#include "tiled_internal.h"

using namespace pem;

// ------------------------------------------------------------------------------------------
// order maps
// ------------------------------------------------------------------------------------------
// Row-major order, 16 lanes per tile (lane = local row, the shape of conv_tile_meta_kernel).  FILL = false: the row's
// population into its (tile row, local row, tile) slot.  FILL = true: the scanned slot is the position in V of the row's
// first entry in this tile; its entries follow.
template <bool FILL>
__global__ void __launch_bounds__(256) vmap_rows_kernel(const long long *__restrict__ tile_keys, const int *__restrict__ tile_rowptr,
                                                        const uint32_t *__restrict__ rec, const int *__restrict__ tile_nnz_ptr,
                                                        long long ntiles, int *__restrict__ slots, int *__restrict__ map)
{
    const long long t = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int r = threadIdx.x & 15;
    if (t >= ntiles) return;
    const int R = (int)(tile_keys[t] >> 32);
    const long long b = tile_rowptr[R], n = tile_rowptr[R + 1] - b;
    const size_t slot = 16 * (size_t)b + (size_t)(r * n + (t - b));
    const uint32_t w = rec[16 * (size_t)t + r];   // row mask | entries of the rows above << 16
    const int cnt = __popc(w & 0xFFFFu);
    if (!FILL) {
        slots[slot] = cnt;
        return;
    }
    const int src = slots[slot];
    int *dst = map + tile_nnz_ptr[t] + (int)(w >> 16);
    for (int k = 0; k < cnt; ++k) dst[k] = src + k;
}

// Column-major order, 16 lanes per tile in tile-CSC order (p = CSC position, lane = local column).  The k-th entry of column c
// is row r = the k-th set bit of masks_t; in tile storage it sits at (entries of rows < r) + (entries of row r left of c).
template <bool FILL>
__global__ void __launch_bounds__(256) vmap_cols_kernel(const long long *__restrict__ tile_keys, const int *__restrict__ tile_colptr,
                                                        const int *__restrict__ tile_offsets, const uint16_t *__restrict__ masks_t,
                                                        const uint32_t *__restrict__ rec, const int *__restrict__ tile_nnz_ptr,
                                                        long long ntiles, int *__restrict__ slots, int *__restrict__ map)
{
    const long long p = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int c = threadIdx.x & 15;
    if (p >= ntiles) return;
    const long long t = tile_offsets[p];
    const int C = (int)(tile_keys[t] & 0xFFFFFFFFll);
    const long long b = tile_colptr[C], m = tile_colptr[C + 1] - b;
    const size_t slot = 16 * (size_t)b + (size_t)(c * m + (p - b));
    unsigned bits = masks_t[16 * (size_t)t + c];
    if (!FILL) {
        slots[slot] = __popc(bits);
        return;
    }
    int src = slots[slot];
    const int e0 = tile_nnz_ptr[t];
    const unsigned left = (1u << c) - 1u;
    while (bits) {
        const int r = __builtin_ctz(bits);
        bits &= bits - 1u;
        const uint32_t w = rec[16 * (size_t)t + r];
        map[e0 + (int)(w >> 16) + __popc(w & 0xFFFFu & left)] = src++;
    }
}

// entry e of tile t, row r, column c -> its slot in vals_t (conv_vals_t_kernel's formula); 16 lanes per tile, lane = local row
__global__ void __launch_bounds__(256) vmap_t_kernel(const uint32_t *__restrict__ rec, const uint32_t *__restrict__ rec_t,
                                                     const int *__restrict__ tile_nnz_ptr, long long ntiles, int *__restrict__ map_t)
{
    const long long t = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int r = threadIdx.x & 15;
    if (t >= ntiles) return;
    const uint32_t w = rec[16 * (size_t)t + r];
    const int e0 = tile_nnz_ptr[t];
    unsigned bits = w & 0xFFFFu;
    int e = e0 + (int)(w >> 16);
    const unsigned above = (1u << r) - 1u;
    while (bits) {
        const int c = __builtin_ctz(bits);
        bits &= bits - 1u;
        const uint32_t wt = rec_t[16 * (size_t)t + c];
        map_t[e++] = e0 + (int)(wt >> 16) + __popc(wt & 0xFFFFu & above);
    }
}

// ------------------------------------------------------------------------------------------
// refresh: vals[e] = vals_t[map_t[e]] = V[map[e]] (MAPPED) or V[e], four entries per lane (16-byte map loads, 16/32-byte vals
// stores).  A plain copy through registers: every bit pattern (NaN payloads, -0.0, subnormals) arrives unchanged.  Serves
// pem_tiled_set_values* and the refresh of the tilings made from a plan's C (chain.hip) or by select (select.hip).
// ------------------------------------------------------------------------------------------
template <typename VT, bool MAPPED>
__global__ void __launch_bounds__(256) vals_refresh_kernel(const VT *__restrict__ V, const int *__restrict__ map, const int *__restrict__ map_t,
                                                           size_t nnz, VT *__restrict__ vals, VT *__restrict__ vals_t)
{
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t e = 4 * q;
    if (e + 4 <= nnz) {
        const int4 d = reinterpret_cast<const int4 *>(map_t)[q];
        VT v0, v1, v2, v3;
        if constexpr (MAPPED) {
            const int4 s = reinterpret_cast<const int4 *>(map)[q];
            v0 = V[s.x], v1 = V[s.y], v2 = V[s.z], v3 = V[s.w];
        } else {
            v0 = V[e], v1 = V[e + 1], v2 = V[e + 2], v3 = V[e + 3];
        }
        if constexpr (sizeof(VT) == 8) {
            double2 *o = reinterpret_cast<double2 *>(vals + e);
            o[0] = make_double2(v0, v1);
            o[1] = make_double2(v2, v3);
        } else {
            reinterpret_cast<float4 *>(vals + e)[0] = make_float4(v0, v1, v2, v3);
        }
        vals_t[d.x] = v0;
        vals_t[d.y] = v1;
        vals_t[d.z] = v2;
        vals_t[d.w] = v3;
    } else {
        for (size_t i = e; i < nnz; ++i) {
            const VT v = MAPPED ? V[map[i]] : V[i];
            vals[i] = v;
            vals_t[map_t[i]] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
// The maps of one order (and vmap_t) on the first refresh that needs them.  Everything stays on the stream: no read-back.
pem_status pem::ensure_vmap_t(pem_ctx *ctx, pem_tiled *T)
{
    if (T->vmap_t_ready) return PEM_OK;
    const size_t nnz = (size_t)T->nnz, nt = (size_t)T->ntiles;
    PEM_TRY(T->vmap_t.reserve(sizeof(int) * (nnz + 4)));
    PEM_LAUNCH(ctx, vmap_t_kernel, grid_for(16 * nt, 256), 256, T->tile_rec.as<uint32_t>(), T->tile_rec_t.as<uint32_t>(), T->tile_nnz_ptr.as<int>(),
               (long long)nt, T->vmap_t.as<int>());
    T->vmap_t_ready = true;
    return PEM_OK;
}

// The mapped form keeps the name tools/numeric_pass.py looks its time up by
template <typename VT>
static void launch_gather(pem_ctx *ctx, pem_tiled *T, const VT *src, const int *map)
{
    const size_t nnz = (size_t)T->nnz;
    const unsigned grid = grid_for((nnz + 3) / 4, 256);
    const bool f32 = sizeof(VT) == 4;
    if (map)
        PEM_LAUNCH_NAMED(ctx, f32 ? "vals_refresh_kernel<float>" : "vals_refresh_kernel<double>", (vals_refresh_kernel<VT, true>), grid, 256, src,
                         map, T->vmap_t.as<int>(), nnz, T->vals.as<VT>(), T->vals_t.as<VT>());
    else
        PEM_LAUNCH_NAMED(ctx, f32 ? "vals_refresh_kernel<float, identity>" : "vals_refresh_kernel<double, identity>", (vals_refresh_kernel<VT, false>),
                         grid, 256, src, nullptr, T->vmap_t.as<int>(), nnz, T->vals.as<VT>(), T->vals_t.as<VT>());
}

void pem::refresh_gather(pem_ctx *ctx, pem_tiled *T, const void *src, const int *map)
{
    if (T->value_bytes == 4)
        launch_gather(ctx, T, static_cast<const float *>(src), map);
    else
        launch_gather(ctx, T, static_cast<const double *>(src), map);
}

static pem_status ensure_maps(pem_ctx *ctx, pem_tiled *T, int order)
{
    const size_t nnz = (size_t)T->nnz, nt = (size_t)T->ntiles;
    const unsigned grid = grid_for(16 * nt, 256);
    PEM_TRY(ensure_vmap_t(ctx, T));
    if (T->vmap_ready[order]) return PEM_OK;
    DevBuf slots;   // (tile row, local row, tile) resp. (tile column, local column, tile) populations -> their exclusive scan
    PEM_TRY(arena_phase(ctx->arena, {{&T->vmap[order], sizeof(int) * (nnz + 4)}, {&slots, sizeof(int) * (16 * nt + 4)}}));
    PEM_TRY(T->vmap[order].reserve(sizeof(int) * (nnz + 4)));
    PEM_TRY(slots.reserve(sizeof(int) * (16 * nt + 4)));
    int *map = T->vmap[order].as<int>(), *s = slots.as<int>();
    if (order == PEM_VALUES_ROW_MAJOR) {
        PEM_LAUNCH(ctx, vmap_rows_kernel<false>, grid, 256, T->tile_keys.as<long long>(), T->tile_rowptr.as<int>(), T->tile_rec.as<uint32_t>(),
                   T->tile_nnz_ptr.as<int>(), (long long)nt, s, map);
        PEM_TRY(exclusive_scan_i32(ctx, s, s, 16 * nt, nullptr));
        PEM_LAUNCH(ctx, vmap_rows_kernel<true>, grid, 256, T->tile_keys.as<long long>(), T->tile_rowptr.as<int>(), T->tile_rec.as<uint32_t>(),
                   T->tile_nnz_ptr.as<int>(), (long long)nt, s, map);
    } else {
        PEM_LAUNCH(ctx, vmap_cols_kernel<false>, grid, 256, T->tile_keys.as<long long>(), T->tile_colptr.as<int>(), T->tile_offsets.as<int>(),
                   T->masks_t.as<uint16_t>(), T->tile_rec.as<uint32_t>(), T->tile_nnz_ptr.as<int>(), (long long)nt, s, map);
        PEM_TRY(exclusive_scan_i32(ctx, s, s, 16 * nt, nullptr));
        PEM_LAUNCH(ctx, vmap_cols_kernel<true>, grid, 256, T->tile_keys.as<long long>(), T->tile_colptr.as<int>(), T->tile_offsets.as<int>(),
                   T->masks_t.as<uint16_t>(), T->tile_rec.as<uint32_t>(), T->tile_nnz_ptr.as<int>(), (long long)nt, s, map);
    }
    T->vmap_ready[order] = true;
    return PEM_OK;
}

// dV: device values in `order`, value_bytes wide.  host != nullptr: upload from there first (into dV's staging buffer) and wait.
static pem_status set_values(pem_ctx *ctx, pem_tiled *T, const void *host, const void *dV, int order, int value_bytes, const char *fn)
{
    if (!ctx || !T) {
        set_error("%s: null context or tiling", fn);
        return PEM_E_INVALID;
    }
    if (order != PEM_VALUES_ROW_MAJOR && order != PEM_VALUES_COL_MAJOR) {
        set_error("%s: order %d is neither PEM_VALUES_ROW_MAJOR (0) nor PEM_VALUES_COL_MAJOR (1)", fn, order);
        return PEM_E_INVALID;
    }
    if (T->value_bytes != value_bytes) {
        set_error("%s: the tiling holds %s values; use the %s entry points", fn, T->value_bytes == 4 ? "fp32" : "fp64",
                  T->value_bytes == 4 ? "_f32" : "fp64");
        return PEM_E_INVALID;
    }
    if (T->nnz == 0) return PEM_OK;
    if (!(host ? host : dV)) {
        set_error("%s: null values for a tiling of %lld entries", fn, (long long)T->nnz);
        return PEM_E_INVALID;
    }
    PEM_ENTER(ctx);
    const size_t nnz = (size_t)T->nnz;
    if (host) {
        PEM_TRY(zero_flags(ctx));
        DevBuf &stage = ctx->tmp[1];   // context-owned, grow-only: a repeat refresh allocates nothing
        PEM_TRY(stage.reserve((size_t)value_bytes * (nnz + 1)));
        PEM_HIP(hipMemcpyAsync(stage.p, host, (size_t)value_bytes * nnz, hipMemcpyHostToDevice, ctx->stream));
        dV = stage.p;
    }
    PEM_TRY(ensure_maps(ctx, T, order));
    refresh_gather(ctx, T, dV, T->vmap[order].as<int>());
    ++T->value_version;
    if (!host) return PEM_OK;   // device form: a failure surfaces at pem_ctx_synchronize
    int hf[NUM_FLAGS];
    PEM_TRY(read_flags(ctx, hf));   // (synchronises)
    if (hf[FLAG_INTERNAL]) T->vmap_ready[order] = false;   // the map's scan gave up: the map and the values just written are not valid
    return check_internal(hf);
}

extern "C" pem_status pem_tiled_set_values(pem_ctx *ctx, pem_tiled *t, const double *V, int order)
{
    return set_values(ctx, t, V, nullptr, order, 8, "pem_tiled_set_values");
}
extern "C" pem_status pem_tiled_set_values_device(pem_ctx *ctx, pem_tiled *t, const double *dV, int order)
{
    return set_values(ctx, t, nullptr, dV, order, 8, "pem_tiled_set_values_device");
}
extern "C" pem_status pem_tiled_set_values_f32(pem_ctx *ctx, pem_tiled *t, const float *V, int order)
{
    return set_values(ctx, t, V, nullptr, order, 4, "pem_tiled_set_values_f32");
}
extern "C" pem_status pem_tiled_set_values_device_f32(pem_ctx *ctx, pem_tiled *t, const float *dV, int order)
{
    return set_values(ctx, t, nullptr, dV, order, 4, "pem_tiled_set_values_device_f32");
}
