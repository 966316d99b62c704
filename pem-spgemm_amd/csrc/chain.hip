// chain.hip -- chained products: the C of a plan as a new tiling (C or C^T) built on the device, and the refresh of such a
// tiling's values from the plan (include/pem_spgemm.h, pem_tiled_from_cplan / pem_tiled_set_values_from_cplan).
//
// C is already a tiled matrix in the tiling's own order: its tiles ascend by (tile row, tile column) and its entries are
// row-major inside a tile.  So no entry-level sort is needed -- the route to the tile payload the conversion and the cache
// loader derive everything else from (derive_tiled, convert.hip):
//   chain_flag_kernel + scan   C tiles that hold entries -> their index in the tiling (PEM_OPT_PRUNE = 0 and masked plans can
//                              leave empty tiles in C's list; a tiling holds 1..256 entries per tile).  Empty tiles hold no
//                              entries, so a kept tile's first entry is already its offset in the tiling: c_vals is vals as is.
//   chain_scatter_kernel       16 lanes per C tile (lane = tile row r): tile key + entry offset, the (r<<4|c) bytes decoded from
//                              c_mask, and the exclusive scan of the tile-head flags written directly (entry e of kept tile j:
//                              j at the tile's first entry, j + 1 after it) -- so no head flags and no scan over the entries.
//                              The row loop is the candidate-tile route's write_row_bits (tiled_internal.h) without values.
//   vals                       one device copy of c_vals.
// C^T: C's tiling first (its tile CSC lists C's tiles in column order and its vals_t holds each tile's entries column-major),
// then chain_count_t_kernel + scan give C^T's entry offsets and chain_gather_t_kernel writes C^T's payload: tiles in C's CSC
// order, (c<<4|r) in (c, r) order, values from vals_t.  derive_tiled once more.
//
// Refresh: for C, vals = c_vals; for C^T, vals = c_vals gathered through the derivation's map (the position of every entry's value
// in c_vals, built on the first refresh by chain_cmap_kernel).  vals_t through the tiling's vmap_t.  One kernel, values.hip's
// refresh_gather (vals_refresh_kernel, identity or mapped form), stream-ordered, no read-back.
#include "spgemm_internal.h"
#include "tiled_internal.h"

using namespace pem;

// ------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------
// keep[t] = C tile t holds an entry
__global__ void chain_flag_kernel(const int *__restrict__ c_tile_nnz_ptr, long long ntc, int *__restrict__ keep)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < ntc) keep[t] = c_tile_nnz_ptr[t + 1] > c_tile_nnz_ptr[t];
}

// 16 lanes per C tile, lane = tile row r.  idx = exclusive scan of keep (idx[ntc] = kept tiles).  c_mask16[16 t + (r ^ 1)] is
// row r's column mask (PEM_C_MASK: (row 2q) << 16 | row 2q+1 per 32-bit word).
__global__ void __launch_bounds__(256) chain_scatter_kernel(const int *__restrict__ c_tile_nnz_ptr, const int *__restrict__ c_tile_rowidx,
                                                            const int *__restrict__ c_tile_colidx, const uint16_t *__restrict__ c_mask16,
                                                            const int *__restrict__ idx, long long ntc, long long *__restrict__ tile_keys,
                                                            int *__restrict__ tile_nnz_ptr, uint8_t *__restrict__ rowcolidx, int *__restrict__ headx)
{
    const long long t = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int r = threadIdx.x & 15;
    const bool live = t < ntc;   // (every lane of a 16-lane group takes part in the scan below)
    int e0 = 0, e1 = 0;
    unsigned m = 0;
    if (live) {
        e0 = c_tile_nnz_ptr[t];
        e1 = c_tile_nnz_ptr[t + 1];
        if (e1 > e0) m = c_mask16[16 * (size_t)t + (r ^ 1)];
    }
    // (not cand_slots: the offsets are read before the scan here, because the mask load hangs on them, and reading them again
    // after it cost chain_scatter_kernel 2 to 4 % on the MI355X: DESIGN.md, the candidate-tile route)
    const int cnt = __popc(m);
    int inc = cnt;
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) {
        const int v = __shfl_up(inc, d, 16);
        if (r >= d) inc += v;
    }
    if (t == 0 && r == 0) {   // closing offsets: tile_nnz_ptr[T] = nnz, headx[nnz] = T
        const int nt = idx[ntc], nnz = c_tile_nnz_ptr[ntc];
        tile_nnz_ptr[nt] = nnz;
        headx[nnz] = nt;
    }
    if (!live || e1 == e0) return;
    const int j = idx[t];
    if (r == 0) {
        tile_keys[j] = ((long long)c_tile_rowidx[t] << 32) | (long long)(unsigned)c_tile_colidx[t];
        tile_nnz_ptr[j] = e0;
    }
    write_row_bits(m, 0u, r, e0 + (inc - cnt), e0, e1, j, rowcolidx, headx);
}

// C^T's tile q is C's tile at CSC position q: its entry count
__global__ void chain_count_t_kernel(const int *__restrict__ tile_offsets, const int *__restrict__ tile_nnz_ptr, long long nt, int *__restrict__ cnt)
{
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nt) return;
    const int t = tile_offsets[q];
    cnt[q] = tile_nnz_ptr[t + 1] - tile_nnz_ptr[t];
}

// 16 lanes per C^T tile q (= C's tile t at CSC position q), lane = C's local column c = C^T's local row.  Row c of the C^T tile
// is column c of the C tile: rows r of masks_t in ascending order, its values the column's run in vals_t.
template <typename VT>
__global__ void __launch_bounds__(256) chain_gather_t_kernel(const int *__restrict__ tile_offsets, const long long *__restrict__ c_keys,
                                                             const int *__restrict__ c_nnz_ptr, const uint32_t *__restrict__ c_rec_t,
                                                             const VT *__restrict__ c_vals_t, long long nt, const int *__restrict__ nnz_ptr,
                                                             long long *__restrict__ tile_keys, uint8_t *__restrict__ rowcolidx,
                                                             VT *__restrict__ vals, int *__restrict__ headx)
{
    const long long q = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int c = threadIdx.x & 15;
    if (q == 0 && c == 0) headx[nnz_ptr[nt]] = (int)nt;
    if (q >= nt) return;
    const int t = tile_offsets[q];
    if (c == 0) {
        const long long k = c_keys[t];
        tile_keys[q] = ((k & 0xFFFFFFFFll) << 32) | (k >> 32);
    }
    const uint32_t w = c_rec_t[16 * (size_t)t + c];   // rows holding column c | entries in the columns before c << 16
    unsigned bits = w & 0xFFFFu;
    const int e0 = nnz_ptr[q], e1 = nnz_ptr[q + 1];
    int e = e0 + (int)(w >> 16);
    const VT *src = c_vals_t + c_nnz_ptr[t] + (int)(w >> 16);
    while (bits) {
        const int r = __builtin_ctz(bits);
        bits &= bits - 1u;
        if (e < e1) {
            rowcolidx[e] = (uint8_t)((c << 4) | r);
            vals[e] = *src;
            headx[e] = e == e0 ? (int)q : (int)q + 1;
        }
        ++e;
        ++src;
    }
}

// cmap of a C^T tiling T: C's tile q is T's tile at T's CSC position q, and C stores it row-major = T's tile column-major, so
// T's entry (r', c') finds its value at cbase[q] + (entries of T's columns < c') + (rows < r' holding column c').
// 16 lanes per CSC position q, lane = T's local column c'.  cbase = exclusive scan of the tiles' counts in CSC order.
__global__ void __launch_bounds__(256) chain_cmap_kernel(const int *__restrict__ tile_offsets, const int *__restrict__ tile_nnz_ptr,
                                                         const uint32_t *__restrict__ rec, const uint32_t *__restrict__ rec_t,
                                                         const int *__restrict__ cbase, long long nt, int *__restrict__ cmap)
{
    const long long q = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int c = threadIdx.x & 15;
    if (q >= nt) return;
    const int t = tile_offsets[q];
    const uint32_t wt = rec_t[16 * (size_t)t + c];
    unsigned bits = wt & 0xFFFFu;
    int src = cbase[q] + (int)(wt >> 16);
    const int e0 = tile_nnz_ptr[t];
    const unsigned left = (1u << c) - 1u;
    while (bits) {
        const int r = __builtin_ctz(bits);
        bits &= bits - 1u;
        const uint32_t w = rec[16 * (size_t)t + r];   // row r's mask | entries of the rows above << 16
        cmap[e0 + (int)(w >> 16) + __popc(w & 0xFFFFu & left)] = src++;
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
static pem_status c_current(const pem_cplan *p, const char *fn)
{
    if (p->state < 3) {
        set_error("%s: step 3 has not run on the plan", fn);
        return PEM_E_STATE;
    }
    return c_values_current(p, fn);
}

// C's tiling (the plan's full shape A.rows x B.cols) into T
static pem_status c_tiling(pem_ctx *ctx, const pem_cplan *p, pem_tiled *T)
{
    hipStream_t st = ctx->stream;
    const size_t ntc = (size_t)p->ntiles_c, nnz = (size_t)p->nnz_c;
    PEM_TRY(zero_flags(ctx));
    PEM_TRY(ensure_c_rowidx(ctx, p));   // absolute tile row per C tile
    PEM_TRY(ensure_compact(ctx, p));    // tile column per C tile, reference layout
    DevBuf idx;                         // int per C tile: holds entries -> (scanned) its tile index in T
    PEM_TRY(idx.reserve(sizeof(int) * (ntc + 4)));
    int64_t nt = 0;
    if (ntc) {
        PEM_LAUNCH(ctx, chain_flag_kernel, grid_for(ntc, 256), 256, p->c_tile_nnz_ptr.as<int>(), (long long)ntc, idx.as<int>());
        PEM_TRY(exclusive_scan_i32(ctx, idx.as<int>(), idx.as<int>(), ntc, ctx->d_scalars));
        PEM_TRY(read_scalars(ctx, ctx->d_scalars, 1, &nt));
        int hf[NUM_FLAGS];
        PEM_TRY(read_flags(ctx, hf));
        PEM_TRY(check_internal(hf));
    }
    set_tiled_shape(T, p->A->value_bytes, p->A->rows, p->B->cols);
    T->nnz = (int64_t)nnz;
    T->ntiles = nt;
    const int bits_tr = bits_for((uint64_t)T->tile_rows), bits_tc = bits_for((uint64_t)T->tile_cols);
    PEM_TRY(reserve_payload(ctx, T));
    int *headx;
    PEM_TRY(begin_payload(ctx, T, &headx));
    if (ntc)
        PEM_LAUNCH(ctx, chain_scatter_kernel, grid_for(16 * ntc, 256), 256, p->c_tile_nnz_ptr.as<int>(), p->c_tile_rowidx.as<int>(),
                   p->c_tile_colidx.as<int>(), p->c_mask.as<uint16_t>(), idx.as<int>(), (long long)ntc, T->tile_keys.as<long long>(),
                   T->tile_nnz_ptr.as<int>(), T->rowcolidx.as<uint8_t>(), headx);
    if (nnz) PEM_HIP(hipMemcpyAsync(T->vals.p, p->c_vals.p, (size_t)T->value_bytes * nnz, hipMemcpyDeviceToDevice, st));
    return derive_tiled(ctx, T, headx, bits_tr, bits_tc);
}

// C^T from C's tiling Tc
template <typename VT>
static pem_status transposed_tiling_t(pem_ctx *ctx, const pem_tiled *Tc, pem_tiled *T)
{
    const size_t nt = (size_t)Tc->ntiles;
    set_tiled_shape(T, Tc->value_bytes, Tc->cols, Tc->rows);
    T->nnz = Tc->nnz;
    T->ntiles = Tc->ntiles;
    const int bits_tr = bits_for((uint64_t)T->tile_rows), bits_tc = bits_for((uint64_t)T->tile_cols);
    PEM_TRY(reserve_payload(ctx, T));
    DevBuf cnt;
    PEM_TRY(cnt.reserve(sizeof(int) * (nt + 4)));
    int *headx;   // (ctx->tmp[0]: Tc's head scan there is no longer read, derive_tiled synchronised)
    PEM_TRY(begin_payload(ctx, T, &headx));
    if (nt) {
        PEM_LAUNCH(ctx, chain_count_t_kernel, grid_for(nt, 256), 256, Tc->tile_offsets.as<int>(), Tc->tile_nnz_ptr.as<int>(), (long long)nt,
                   cnt.as<int>());
        PEM_TRY(exclusive_scan_i32(ctx, cnt.as<int>(), T->tile_nnz_ptr.as<int>(), nt, nullptr));
        PEM_LAUNCH(ctx, chain_gather_t_kernel<VT>, grid_for(16 * nt, 256), 256, Tc->tile_offsets.as<int>(), Tc->tile_keys.as<long long>(),
                   Tc->tile_nnz_ptr.as<int>(), Tc->tile_rec_t.as<uint32_t>(), Tc->vals_t.as<VT>(), (long long)nt, T->tile_nnz_ptr.as<int>(),
                   T->tile_keys.as<long long>(), T->rowcolidx.as<uint8_t>(), T->vals.as<VT>(), headx);
    }
    PEM_TRY(derive_tiled(ctx, T, headx, bits_tr, bits_tc));
    int hf[NUM_FLAGS];
    PEM_TRY(read_flags(ctx, hf));   // (the scan of the entry offsets gave up: nothing behind it is valid)
    return check_internal(hf);
}

pem_status pem::transposed_tiling(pem_ctx *ctx, const pem_tiled *Tc, pem_tiled *T)
{
    return Tc->value_bytes == 4 ? transposed_tiling_t<float>(ctx, Tc, T) : transposed_tiling_t<double>(ctx, Tc, T);
}

// C's tiling into T, or C^T's from a C tiling of its own (freed once C^T is built)
static pem_status cplan_build(pem_ctx *ctx, const pem_cplan *plan, int transpose, pem_tiled *T)
{
    T->derived.kind = Derivation::CPLAN;
    T->derived.src[0] = plan->serial;
    T->derived.op = transpose;
    if (!transpose) return c_tiling(ctx, plan, T);
    std::unique_ptr<pem_tiled> Tc(new pem_tiled());
    pem_status s = c_tiling(ctx, plan, Tc.get());
    if (s == PEM_OK) s = transposed_tiling(ctx, Tc.get(), T);
    (void)hipStreamSynchronize(ctx->stream);   // (C's tiling goes back to the arena)
    return s;
}

extern "C" pem_status pem_tiled_from_cplan(pem_ctx *ctx, const pem_cplan *plan, int transpose, pem_tiled **out)
{
    const char *fn = "pem_tiled_from_cplan";
    if (!ctx || !plan || !out) {
        set_error("%s: null context, plan or output", fn);
        return PEM_E_INVALID;
    }
    *out = nullptr;
    if (transpose != 0 && transpose != 1) {
        set_error("%s: transpose must be 0 or 1, not %d", fn, transpose);
        return PEM_E_INVALID;
    }
    PEM_TRY(c_current(plan, fn));
    return build_derived(ctx, out, [&](pem_tiled *T) { return cplan_build(ctx, plan, transpose, T); });
}

// the map of a C^T tiling on its first refresh: counts in CSC order, scan, fill.  Stream-ordered, no read-back.
pem_status pem::build_transpose_map(pem_ctx *ctx, pem_tiled *T)
{
    const size_t nnz = (size_t)T->nnz, nt = (size_t)T->ntiles;
    DevBuf &cmap = T->derived.map, cbase;
    PEM_TRY(arena_phase(ctx->arena, {{&cmap, sizeof(int) * (nnz + 4)}, {&cbase, sizeof(int) * (nt + 4)}}));
    PEM_TRY(cmap.reserve(sizeof(int) * (nnz + 4)));
    PEM_TRY(cbase.reserve(sizeof(int) * (nt + 4)));
    if (nt) {
        PEM_LAUNCH(ctx, chain_count_t_kernel, grid_for(nt, 256), 256, T->tile_offsets.as<int>(), T->tile_nnz_ptr.as<int>(), (long long)nt,
                   cbase.as<int>());
        PEM_TRY(exclusive_scan_i32(ctx, cbase.as<int>(), cbase.as<int>(), nt, nullptr));
        PEM_LAUNCH(ctx, chain_cmap_kernel, grid_for(16 * nt, 256), 256, T->tile_offsets.as<int>(), T->tile_nnz_ptr.as<int>(),
                   T->tile_rec.as<uint32_t>(), T->tile_rec_t.as<uint32_t>(), cbase.as<int>(), (long long)nt, cmap.as<int>());
    }
    return PEM_OK;
}

extern "C" pem_status pem_tiled_set_values_from_cplan(pem_ctx *ctx, pem_tiled *t, const pem_cplan *plan)
{
    const char *fn = "pem_tiled_set_values_from_cplan";
    if (!ctx || !t || !plan) {
        set_error("%s: null context, tiling or plan", fn);
        return PEM_E_INVALID;
    }
    if (t->derived.kind != Derivation::CPLAN || t->derived.src[0] != plan->serial) {
        set_error("%s: the tiling was not made from this plan by pem_tiled_from_cplan", fn);
        return PEM_E_INVALID;
    }
    PEM_TRY(c_current(plan, fn));
    if (plan->nnz_c != t->nnz) {
        set_error("%s: the plan's C has %lld entries, the tiling %lld", fn, (long long)plan->nnz_c, (long long)t->nnz);
        return PEM_E_INVALID;
    }
    const bool tr = t->derived.op != 0;   // C^T: through the map; C: c_vals as it is
    return refresh_derived(
        ctx, t, [&] { return tr ? build_transpose_map(ctx, t) : PEM_OK; },
        [&] { refresh_gather(ctx, t, plan->c_vals.p, tr ? t->derived.map.as<int>() : nullptr); });
}
