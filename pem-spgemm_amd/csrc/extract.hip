// extract.hip -- the operations that re-index a tiling (include/pem_spgemm.h): R = A(I, J) (pem_tiled_extract,
// pem_tiled_extract_device), R = A^T (pem_tiled_transpose) and their refreshes (pem_tiled_set_values_from_extract / _from_transpose).
//
// Transpose is chain.hip's transposed_tiling: A's tile CSC lists its tiles in A^T's order and vals_t holds each tile column-major.
//
// Extract is built from one tile-native routine, the row gather G = A(I, :), and the transpose:
//   A(I, :)  = gather                         A(:, J) = (gather of A^T by J)^T
//   A(I, J)  = (gather of (A(I, :))^T by J)^T
// so repeated and unordered indices work on both sides alike, and a null list skips its stages.
//
// Row gather.  Row r of a tile is one 16-bit mask in tile_rec and a contiguous run of values, so whole rows move without
// touching the column tiling.  Output tile row P holds the output rows 16P .. 16P+15 with the source rows s_r = I[16P + r]:
//   ex_slots_kernel   16 lanes per output tile row (lane = r).  Lane r is a LEADER when no lane below it reads the same source tile
//                     row; a leader's slot gets the length of that tile row's tile list, every other slot 0.  The scan of the slots
//                     places the concatenated lists: the candidates of P.  Indices are range-checked here (FLAG_RANGE).
// From there on it is the candidate-tile route, which this unit defines for kron.hip and concat.hip too (tiled_internal.h:
// check_candidates, tiling_from_candidates; on the device cand_key, cand_count, cand_slots, cand_tile_head, write_row_bits) with these stages:
//   ex_cand_kernel    (emit) one lane per candidate: its slot by a binary search in the scanned slots, its key (P, tile column).
//   sort              only where some output tile row has two leaders or more (a second scan, of the non-first leaders, tells).
//                     With one leader per output tile row -- I == NULL, aligned ranges, one index repeated -- the concatenation is
//                     already A's order and nothing is sorted or merged.
//   ex_count_kernel   (count) lane r of a candidate: the source tile by mask_find_tile, one tile_rec word.
//   ex_fill_kernel    (fill) the same word again: the row's mask as it is, its values the source run.
// The route: the candidate keys; radix_sort_u64_u32 over the candidate TILES' keys where asked (duplicates end up adjacent and the
// count drops all but the first); the count, 16 lanes per candidate, whose 16-lane sum is the tile's entries and a non-empty flag;
// the pair scan to entry offsets and tile ids, the totals read back and checked (check_result_entries) before the payload is
// allocated; the fill, 16 lanes per candidate again: tile_keys, tile_nnz_ptr, the (r << 4) | c bytes, the tile-head scan written
// directly and the values, each written once; derive_tiled for everything else.
// No kernel walks a tile row serially: every candidate is a lane (ex_cand_kernel) or a 16-lane group, whatever its tile row's length.
//
// Refresh: both patterns are independent of A's values.  The first call builds an int32 per entry, its slot in A's vals -- for a
// transpose chain.hip's map, for an extract by decoding every entry's (p, q), finding A's tile at (I[p] >> 4, J[q] >> 4) and taking
// src_slot there (the device copies of I and J stay with the tiling) -- and every call is values.hip's refresh_gather.
#include "spgemm_internal.h"
#include "tiled_internal.h"
#include <climits>
#include <vector>

using namespace pem;

// ------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------
// the source index of output index p (a null list is the identity)
__device__ __forceinline__ int ex_src(const int *__restrict__ L, const long long p)
{
    return L ? L[p] : (int)p;
}

// 16 lanes per output tile row P, lane = local row r.  slots[16P + r] = tiles of source tile row I[16P + r] >> 4 where lane r leads
// it, else 0; later[16P + r] = 1 for a leader that is not its tile row's first.  np = output tile rows.  holes (scatter_tiling
// only): a negative index is an output row without entries, not a range error.
__global__ void __launch_bounds__(256) ex_slots_kernel(const int *__restrict__ I, long long ni, int a_rows, const int *__restrict__ a_rowptr,
                                                       long long np, int holes, int *__restrict__ slots, int *__restrict__ later,
                                                       int *__restrict__ flags)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int r = threadIdx.x & 15;
    const bool live = (g >> 4) < np;   // (every lane of a 16-lane group takes part in the shuffles below)
    int S = -1;
    if (live && g < ni) {
        const int s = ex_src(I, g);
        if (s >= 0 && s < a_rows)
            S = s >> 4;
        else if (!(holes && s < 0))
            flags[FLAG_RANGE] = 1;   // (the lane takes no part: a bad index is never an address)
    }
    bool dup = false, before = false;
#pragma unroll
    for (int d = 1; d < 16; ++d) {
        const int v = __shfl_up(S, d, 16);
        if (r >= d) {
            dup |= v == S;
            before |= v >= 0;
        }
    }
    if (!live) return;
    const bool lead = S >= 0 && !dup;
    slots[g] = lead ? a_rowptr[S + 1] - a_rowptr[S] : 0;
    later[g] = lead && before;
}

// one lane per candidate c: its slot g (coff[g] <= c < coff[g + 1]; coff = the scanned slots, ns + 1 values), then its key
// (output tile row << bits_tc) | tile column
__global__ void ex_cand_kernel(const int *__restrict__ I, const int *__restrict__ a_rowptr, const int *__restrict__ a_colidx,
                               const int *__restrict__ coff, long long ns, long long ncand, int bits_tc, uint64_t *__restrict__ keys)
{
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncand) return;
    long long lo = 0, hi = ns - 1;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (coff[mid + 1] <= c)
            lo = mid + 1;
        else
            hi = mid;
    }
    const int S = ex_src(I, lo) >> 4;   // (a slot with candidates belongs to a leader: its index passed the range check)
    const int tc = a_colidx[a_rowptr[S] + (int)(c - coff[lo])];
    keys[c] = ((uint64_t)(lo >> 4) << bits_tc) | (uint64_t)(unsigned)tc;
}

// what lane r of candidate k reads: A's tile at (source tile row, k.Q) and the tile_rec word of the source row there (0: none).
// A duplicate reads nothing; so does a hole (a negative index, scatter_tiling).
struct ExRow {
    int t;
    uint32_t rec;
};
__device__ __forceinline__ ExRow ex_row(const CandKey &k, const int r, const int *__restrict__ I, const long long ni,
                                        const int *__restrict__ a_rowptr, const int *__restrict__ a_colidx, const uint32_t *__restrict__ a_rec)
{
    ExRow x = {-1, 0u};
    if (k.dup) return x;
    const long long p = 16 * k.P + r;
    if (p >= ni) return x;
    const int s = ex_src(I, p);
    if (s < 0) return x;
    x.t = mask_find_tile(a_rowptr, a_colidx, s >> 4, (int)k.Q);
    if (x.t >= 0) x.rec = a_rec[16 * (size_t)x.t + (s & 15)];
    return x;
}

// 16 lanes per candidate, lane = local row r: cnt[c] = the output tile's entries, flag[c] = it has any
__global__ void __launch_bounds__(256) ex_count_kernel(const uint64_t *__restrict__ keys, long long ncand, const int *__restrict__ I, long long ni,
                                                       const int *__restrict__ a_rowptr, const int *__restrict__ a_colidx,
                                                       const uint32_t *__restrict__ a_rec, int bits_tc, int *__restrict__ cnt,
                                                       int *__restrict__ flag)
{
    const long long c = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int r = threadIdx.x & 15;
    int n = 0;
    if (c < ncand) n = __popc(ex_row(cand_key(keys, c, bits_tc), r, I, ni, a_rowptr, a_colidx, a_rec).rec & 0xFFFFu);
    cand_count(n, c, ncand, r, cnt, flag);
}

// 16 lanes per candidate, lane = local row r.  Row r of output tile rid[c] is the source row's mask; its values are the source run.
template <typename VT>
__global__ void __launch_bounds__(256) ex_fill_kernel(const uint64_t *__restrict__ keys, long long ncand, const int *__restrict__ I, long long ni,
                                                      const int *__restrict__ a_rowptr, const int *__restrict__ a_colidx,
                                                      const uint32_t *__restrict__ a_rec, const int *__restrict__ a_ptr,
                                                      const VT *__restrict__ a_vals, int bits_tc, const int *__restrict__ roff,
                                                      const int *__restrict__ rid, long long *__restrict__ tile_keys,
                                                      int *__restrict__ tile_nnz_ptr, uint8_t *__restrict__ rowcolidx, int *__restrict__ headx,
                                                      VT *__restrict__ vals)
{
    const long long c = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int r = threadIdx.x & 15;
    ExRow x = {-1, 0u};
    CandKey k = {0, 0, false};
    if (c < ncand) {
        k = cand_key(keys, c, bits_tc);
        x = ex_row(k, r, I, ni, a_rowptr, a_colidx, a_rec);
    }
    const unsigned m = x.rec & 0xFFFFu;
    cand_slots(c, ncand, r, __popc(m), roff, rid, tile_nnz_ptr, headx, [&](const CandSlots &s) {
        cand_tile_head(r, s, k.P, k.Q, tile_keys, tile_nnz_ptr);
        if (!m) return;
        const VT *src = a_vals + a_ptr[x.t] + (int)(x.rec >> 16);
        write_row_bits(m, 0u, r, s.e, s.e0, s.e1, s.t, rowcolidx, headx, vals, [&](unsigned) { return *src++; });
    });
}

// the refresh map of an extract, once.  Entry (p, q) of R is entry (I[p], J[q]) of A: A's tile there by mask_find_tile, its slot by
// src_slot.
__global__ void __launch_bounds__(256) ex_map_kernel(const long long *__restrict__ r_keys, long long nt, const int *__restrict__ r_ptr,
                                                     const uint8_t *__restrict__ r_rci, const int *__restrict__ I, const int *__restrict__ J,
                                                     const int *__restrict__ a_rowptr, const int *__restrict__ a_colidx,
                                                     const int *__restrict__ a_ptr, const uint32_t *__restrict__ a_rec, int *__restrict__ map)
{
    for_tile_entries(r_keys, nt, r_ptr, r_rci, [&](const int e, const long long p, const long long q) {
        const int si = ex_src(I, p), sj = ex_src(J, q);
        const int t = mask_find_tile(a_rowptr, a_colidx, si >> 4, sj >> 4);
        map[e] = t >= 0 ? src_slot(a_ptr[t], a_rec[16 * (size_t)t + (si & 15)], (unsigned)(sj & 15)) : 0;
    });
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
// G = A(I, :) for a device list dI of ni checked-on-device indices (null: every row in order, ni = A's rows).  The flags were zeroed
// by the caller.  holes: a negative index is an empty output row (scatter_tiling).
template <typename VT>
static pem_status gather_rows(pem_ctx *ctx, const pem_tiled *A, const int *dI, int64_t ni, bool holes, pem_tiled *G, const char *fn)
{
    set_tiled_shape(G, A->value_bytes, (int)ni, A->cols);
    const size_t np = (size_t)G->tile_rows, ns = 16 * np;
    const int bits_tc = bits_for((uint64_t)G->tile_cols);
    DevBuf slots, later;   // per (output tile row, local row): candidates it leads -> their offset; a non-first leader
    PEM_TRY(slots.reserve(sizeof(int) * (ns + 4)));
    PEM_TRY(later.reserve(sizeof(int) * (ns + 4)));
    PEM_LAUNCH(ctx, ex_slots_kernel, grid_for(ns, 256), 256, dI, (long long)ni, A->rows, A->tile_rowptr.as<int>(), (long long)np, holes ? 1 : 0,
               slots.as<int>(), later.as<int>(), ctx->d_flags);
    PEM_TRY(exclusive_scan_i32_pair(ctx, slots.as<int>(), later.as<int>(), ns, ctx->d_scalars, ctx->d_scalars + 1));
    int64_t tot[2] = {0, 0};
    PEM_TRY(check_candidates(ctx, 2, tot, fn, [&](const int *hf) {
        if (!hf[FLAG_RANGE]) return PEM_OK;
        set_error("%s: an index is negative or not below the dimension (%d)", fn, A->rows);
        return PEM_E_INVALID;
    }));
    const size_t ncand = (size_t)tot[0];
    const bool merge = tot[1] != 0;   // some output tile row draws on two source tile rows or more: only then are the candidates sorted
    const long long nc = (long long)ncand;
    const int *a_rowptr = A->tile_rowptr.as<int>(), *a_colidx = A->tile_colidx.as<int>();
    const uint32_t *a_rec = A->tile_rec.as<uint32_t>();
    CandidateStages st;
    st.emit = [&](uint64_t *keys) {
        PEM_LAUNCH(ctx, ex_cand_kernel, grid_for(ncand, 256), 256, dI, a_rowptr, a_colidx, slots.as<int>(), (long long)ns, nc, bits_tc, keys);
    };
    st.count = [&](const uint64_t *keys, int *cnt, int *flag) {
        PEM_LAUNCH(ctx, ex_count_kernel, grid_for(16 * ncand, 256), 256, keys, nc, dI, (long long)ni, a_rowptr, a_colidx, a_rec, bits_tc, cnt, flag);
    };
    st.fill = [&](const uint64_t *keys, const int *roff, const int *rid, int *headx) {
        PEM_LAUNCH(ctx, ex_fill_kernel<VT>, grid_for(16 * ncand, 256), 256, keys, nc, dI, (long long)ni, a_rowptr, a_colidx, a_rec,
                   A->tile_nnz_ptr.as<int>(), A->vals.as<VT>(), bits_tc, roff, rid, G->tile_keys.as<long long>(), G->tile_nnz_ptr.as<int>(),
                   G->rowcolidx.as<uint8_t>(), headx, G->vals.as<VT>());
    };
    return tiling_from_candidates(ctx, G, fn, ncand, merge, -1, "", st);
}

// ---- the candidate-tile route's host half (tiled_internal.h) ----
pem_status pem::check_candidates(pem_ctx *ctx, int ntot, int64_t *tot, const char *fn, const std::function<pem_status(const int *flags)> &refuse)
{
    PEM_TRY(read_scalars(ctx, ctx->d_scalars, ntot, tot));
    int hf[NUM_FLAGS];
    PEM_TRY(read_flags(ctx, hf));
    if (refuse) PEM_TRY(refuse(hf));
    if (hf[FLAG_OVERFLOW] || tot[0] > 0x7FFFFFFFll) {
        set_error("%s: the result's tiles exceed the int32 index range", fn);
        return PEM_E_OVERFLOW;
    }
    return check_internal(hf);
}

pem_status pem::tiling_from_candidates(pem_ctx *ctx, pem_tiled *R, const char *fn, size_t ncand, bool sort, int64_t expect_nnz,
                                       const char *expect_what, const CandidateStages &stages)
{
    const int bits_tr = bits_for((uint64_t)R->tile_rows), bits_tc = bits_for((uint64_t)R->tile_cols);
    DevBuf k0, k1, v0, v1, roff, rid;   // candidate keys (and the sort's other half and payloads); per candidate: count -> entry offset, flag -> tile id
    PEM_TRY(k0.reserve(sizeof(uint64_t) * (ncand + 1)));
    PEM_TRY(roff.reserve(sizeof(int) * (ncand + 4)));
    PEM_TRY(rid.reserve(sizeof(int) * (ncand + 4)));
    uint64_t *keys = k0.as<uint64_t>();
    if (ncand) {
        stages.emit(keys);
        if (sort) {   // duplicates end up adjacent, and the count drops all but the first
            PEM_TRY(k1.reserve(sizeof(uint64_t) * (ncand + 1)));
            PEM_TRY(v0.reserve(sizeof(uint32_t) * (ncand + 1)));
            PEM_TRY(v1.reserve(sizeof(uint32_t) * (ncand + 1)));
            PEM_HIP(hipMemsetAsync(v0.p, 0, sizeof(uint32_t) * ncand, ctx->stream));   // (the payload is not used)
            uint32_t *pv;
            PEM_TRY(radix_sort_u64_u32(ctx, k0.as<uint64_t>(), k1.as<uint64_t>(), v0.as<uint32_t>(), v1.as<uint32_t>(), ncand, bits_tr + bits_tc,
                                       &keys, &pv));
        }
        stages.count(keys, roff.as<int>(), rid.as<int>());
    }
    PEM_TRY(exclusive_scan_i32_pair(ctx, roff.as<int>(), rid.as<int>(), ncand, ctx->d_scalars, ctx->d_scalars + 1));
    int64_t tot[2] = {0, 0};
    PEM_TRY(read_scalars(ctx, ctx->d_scalars, 2, tot));
    PEM_TRY(check_result_entries(ctx, tot[0], fn));
    if (expect_nnz >= 0 && tot[0] != expect_nnz) {
        set_error("%s: internal: the walk counted %lld entries, not %s %lld", fn, (long long)tot[0], expect_what, (long long)expect_nnz);
        return PEM_E_HIP;
    }
    R->nnz = tot[0];
    R->ntiles = tot[1];
    PEM_TRY(reserve_payload(ctx, R));
    int *headx;
    PEM_TRY(begin_payload(ctx, R, &headx));
    if (ncand) stages.fill(keys, roff.as<int>(), rid.as<int>(), headx);
    return derive_tiled(ctx, R, headx, bits_tr, bits_tc);
}

static pem_status gather(pem_ctx *ctx, const pem_tiled *A, const int *dI, int64_t ni, bool holes, pem_tiled *G, const char *fn)
{
    return A->value_bytes == 4 ? gather_rows<float>(ctx, A, dI, ni, holes, G, fn) : gather_rows<double>(ctx, A, dI, ni, holes, G, fn);
}

// R = A(d[0], d[1]) for device lists of n[0] and n[1] indices (null: all).  The flags were zeroed by the caller.
static pem_status gather_both(pem_ctx *ctx, const pem_tiled *A, const int *const d[2], const int64_t n[2], bool holes, pem_tiled *R, const char *fn)
{
    if (!d[1]) return gather(ctx, A, d[0], n[0], holes, R, fn);
    // the column side: (gather of the transposed rows by J)^T.  Every intermediate goes back to the arena when this returns.
    std::unique_ptr<pem_tiled> G1, T1(new pem_tiled()), G2(new pem_tiled());
    const pem_tiled *src = A;
    if (d[0]) {
        G1.reset(new pem_tiled());
        PEM_TRY(gather(ctx, A, d[0], n[0], holes, G1.get(), fn));
        src = G1.get();
    }
    PEM_TRY(transposed_tiling(ctx, src, T1.get()));
    G1.reset();
    PEM_TRY(gather(ctx, T1.get(), d[1], n[1], holes, G2.get(), fn));
    T1.reset();
    return transposed_tiling(ctx, G2.get(), R);
}

pem_status pem::scatter_tiling(pem_ctx *ctx, const pem_tiled *A, const int *inv_i, int rows, const int *inv_j, int cols, pem_tiled *S, const char *fn)
{
    const int *const d[2] = {inv_i, inv_j};
    const int64_t n[2] = {rows, cols};
    PEM_TRY(zero_flags(ctx));
    pem_status s = gather_both(ctx, A, d, n, true, S, fn);
    (void)hipStreamSynchronize(ctx->stream);   // (the intermediates went back to the arena)
    return s;
}

// R = A(I, J).  The lists (host or device memory, null = all) are first copied into R's derivation, and those copies are what every
// stage reads.
static pem_status extract_build(pem_ctx *ctx, const pem_tiled *A, const int32_t *I, int64_t ni, const int32_t *J, int64_t nj, bool on_device,
                                pem_tiled *R, const char *fn)
{
    R->derived.kind = Derivation::EXTRACT;
    R->derived.src[0] = A->serial;
    PEM_TRY(zero_flags(ctx));
    const int32_t *L[2] = {I, J};
    const int64_t n[2] = {I ? ni : A->rows, J ? nj : A->cols};
    const int *d[2] = {nullptr, nullptr};
    for (int k = 0; k < 2; ++k) {
        if (!L[k]) continue;
        DevBuf &b = R->derived.idx[k];
        PEM_TRY(b.reserve(sizeof(int) * ((size_t)n[k] + 4)));
        PEM_HIP(hipMemcpyAsync(b.p, L[k], sizeof(int) * (size_t)n[k], on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
        d[k] = b.as<int>();
    }
    return gather_both(ctx, A, d, n, false, R, fn);
}

static bool list_size_ok(const void *L, int64_t n, const char *which, const char *fn)
{
    if (L && (n < 1 || n > 0x7FFFFFFFll)) {
        set_error("%s: %s has %lld indices; a list holds 1 .. INT32_MAX of them (a null list is all)", fn, which, (long long)n);
        return false;
    }
    return true;
}

static bool host_list_ok(const int32_t *L, int64_t n, int dim, const char *which, const char *fn)
{
    if (!L) return true;
    for (int64_t k = 0; k < n; ++k)
        if (L[k] < 0 || L[k] >= dim) {
            set_error("%s: %s[%lld] = %d is outside 0 .. %d", fn, which, (long long)k, (int)L[k], dim - 1);
            return false;
        }
    return true;
}

static pem_status extract_entry(pem_ctx *ctx, const pem_tiled *A, const int32_t *I, int64_t ni, const int32_t *J, int64_t nj, bool on_device,
                                pem_tiled **out, const char *fn)
{
    if (!ctx || !A || !out) {
        set_error("%s: null context, operand or output", fn);
        return PEM_E_INVALID;
    }
    *out = nullptr;
    if (!list_size_ok(I, ni, "I", fn) || !list_size_ok(J, nj, "J", fn)) return PEM_E_INVALID;
    if (!on_device && (!host_list_ok(I, ni, A->rows, "I", fn) || !host_list_ok(J, nj, A->cols, "J", fn))) return PEM_E_INVALID;
    return build_derived(ctx, out, [&](pem_tiled *R) {
        pem_status s = extract_build(ctx, A, I, ni, J, nj, on_device, R, fn);
        (void)hipStreamSynchronize(ctx->stream);   // (the intermediates went back to the arena)
        return s;
    });
}

extern "C" pem_status pem_tiled_extract(pem_ctx *ctx, const pem_tiled *A, const int32_t *I, int64_t ni, const int32_t *J, int64_t nj,
                                        pem_tiled **out)
{
    return extract_entry(ctx, A, I, ni, J, nj, false, out, "pem_tiled_extract");
}

extern "C" pem_status pem_tiled_extract_device(pem_ctx *ctx, const pem_tiled *A, const int32_t *dI, int64_t ni, const int32_t *dJ, int64_t nj,
                                               pem_tiled **out)
{
    return extract_entry(ctx, A, dI, ni, dJ, nj, true, out, "pem_tiled_extract_device");
}

// once: every entry's slot in A's vals (nnz + 4 ints, as refresh_gather's four-entry loads want)
static pem_status extract_map(pem_ctx *ctx, pem_tiled *t, const pem_tiled *A)
{
    const size_t nnz = (size_t)t->nnz, nt = (size_t)t->ntiles;
    PEM_TRY(t->derived.map.reserve(sizeof(int) * (nnz + 4)));
    PEM_LAUNCH(ctx, ex_map_kernel, grid_for((nt + 63) / 64 * 64, 256), 256, t->tile_keys.as<long long>(), (long long)nt, t->tile_nnz_ptr.as<int>(),
               t->rowcolidx.as<uint8_t>(), t->derived.idx[0].as<int>(), t->derived.idx[1].as<int>(), A->tile_rowptr.as<int>(),
               A->tile_colidx.as<int>(), A->tile_nnz_ptr.as<int>(), A->tile_rec.as<uint32_t>(), t->derived.map.as<int>());
    return PEM_OK;
}

extern "C" pem_status pem_tiled_set_values_from_extract(pem_ctx *ctx, pem_tiled *t, const pem_tiled *A)
{
    const char *fn = "pem_tiled_set_values_from_extract";
    if (!ctx || !t || !A) {
        set_error("%s: null context, tiling or source", fn);
        return PEM_E_INVALID;
    }
    if (t->derived.kind != Derivation::EXTRACT || t->derived.src[0] != A->serial) {
        set_error("%s: the tiling was not made by pem_tiled_extract from this A", fn);
        return PEM_E_INVALID;
    }
    return refresh_derived(
        ctx, t, [&] { return extract_map(ctx, t, A); }, [&] { refresh_gather(ctx, t, A->vals.p, t->derived.map.as<int>()); });
}

extern "C" pem_status pem_tiled_transpose(pem_ctx *ctx, const pem_tiled *A, pem_tiled **out)
{
    const char *fn = "pem_tiled_transpose";
    if (!ctx || !A || !out) {
        set_error("%s: null context, operand or output", fn);
        return PEM_E_INVALID;
    }
    *out = nullptr;
    return build_derived(ctx, out, [&](pem_tiled *T) {
        T->derived.kind = Derivation::TRANSPOSE;
        T->derived.src[0] = A->serial;
        PEM_TRY(zero_flags(ctx));
        return transposed_tiling(ctx, A, T);
    });
}

extern "C" pem_status pem_tiled_set_values_from_transpose(pem_ctx *ctx, pem_tiled *t, const pem_tiled *A)
{
    const char *fn = "pem_tiled_set_values_from_transpose";
    if (!ctx || !t || !A) {
        set_error("%s: null context, tiling or source", fn);
        return PEM_E_INVALID;
    }
    if (t->derived.kind != Derivation::TRANSPOSE || t->derived.src[0] != A->serial) {
        set_error("%s: the tiling was not made by pem_tiled_transpose from this A", fn);
        return PEM_E_INVALID;
    }
    return refresh_derived(
        ctx, t, [&] { return build_transpose_map(ctx, t); }, [&] { refresh_gather(ctx, t, A->vals.p, t->derived.map.as<int>()); });
}
