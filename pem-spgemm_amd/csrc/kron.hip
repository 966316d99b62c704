// kron.hip -- the Kronecker product of two tilings (include/pem_spgemm.h): R = A (x) B under a binary op (pem_tiled_kron) and its
// refresh (pem_tiled_set_values_from_kron).  With A mA x nA and B mB x nB, R is mA*mB x nA*nB and stores (i*mB + k, j*nB + l)
// exactly where A stores (i, j) and B stores (k, l), with the value op(a, b).
//
// R's order is known in closed form, so no entry is ever sorted.  Row p = i*mB + k of R holds, in ascending column order,
// "for j in A(i, :) ascending, for l in B(k, :) ascending": a tile's row-major order falls out of walking A's row and B's row.  An
// (A entry, B tile) pair covers at most 16 consecutive rows and columns of R, so it reaches at most 2 x 2 tiles of R.  The build
// is the candidate-tile route (tiled_internal.h, extract.hip: sort, pair scan, payload setup, derive_tiled) with these stages:
//   kr_cand_kernel    (emit) one lane per (A entry, B tile) pair -- A's entry coordinates from its tile key and (r << 4) | c byte, the
//                     tile by a binary search in A's tile_nnz_ptr.  First form, before the route: the pair's exact count of R tiles
//                     (1, 2 or 4); after the scan of the counts, second form: their keys (P << bits_tc) | Q.
//   sort              always (the aligned no-sort path was not built: A's entries come in tile order, not row order, so in-order
//                     candidates would need a pass of their own).  Duplicates: a tile of R several pairs reach, every tile when B is
//                     small.
//   kr_count_kernel   (count) lane r of a candidate: row 16P + r -> (i, k) by one division; the at most 16 values of j
//                     whose blocks reach columns 16Q .. 16Q+15 lie in at most two tile columns of A, found once by tile_lower_bound
//                     and read as one 32-bit row mask; for each stored A(i, j) the segment of B's row k lies in at most two tiles of
//                     B, looked up only when its tile column changes (with nB <= 16 once per row), and is shifted into place.  The
//                     row's 16-bit mask is kept per candidate row (rmask, this unit's own buffer); a candidate whose B tile has
//                     nothing in this corner is no tile of R.
//   kr_fill_kernel    (fill) the same walk from the row's first slot (the kept masks' popcounts give it), the values op(a, b) written
//                     once, contiguously per row.
// No atomics, and the order of every array is fixed by the operands alone.  p = i*mB + k and q = j*nB + l reach 2^31 - 1: products
// are formed in 64 bits and narrowed only once they are a tile index, a 4-bit offset or an operand coordinate.
//
// Refresh: the pattern is independent of the values.  The first call builds an int2 per entry -- one lane per entry decodes (p, q)
// from the tile key and byte, divides them into (i, k) and (j, l), and takes src_slot in A's and in B's tile -- and every call is
// ewise.hip's refresh_pairs with the recorded op.
#include "spgemm_internal.h"
#include "tiled_internal.h"
#include <climits>

using namespace pem;

// ------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------
// (what the walks read of an operand is a TileSide, tile_side(T); a row's 32 columns from a tile column on come from row_seg /
// seg_slot: tiled_internal.h, shared with concat.hip)

// One lane per (A entry ea, B tile tb), x = ea * tb_count + tb.  The pair's block of R is rows i*mB + 16K .. (clipped at B's last
// row) and columns j*nB + 16L .. alike: 1 or 2 tile rows times 1 or 2 tile columns.  coff == null: cnt[x] = that count.  Else:
// the keys at coff[x] .. (coff = the scanned counts).
__global__ void __launch_bounds__(256) kr_cand_kernel(const long long *__restrict__ a_keys, const int *__restrict__ a_ptr, long long ta,
                                                      const uint8_t *__restrict__ a_rci, const long long *__restrict__ b_keys, long long tb,
                                                      long long npairs, int mB, int nB, int bits_tc, int *__restrict__ cnt,
                                                      const int *__restrict__ coff, uint64_t *__restrict__ keys)
{
    const long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= npairs) return;
    const long long ea = x / tb;
    const long long key_b = b_keys[x - ea * tb];
    long long lo = 0, hi = ta - 1;   // A's tile of entry ea: a_ptr[lo] <= ea < a_ptr[lo + 1]
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (a_ptr[mid + 1] <= ea)
            lo = mid + 1;
        else
            hi = mid;
    }
    const long long key_a = a_keys[lo];
    const unsigned rc = a_rci[ea];
    const long long i = 16 * (key_a >> 32) + (rc >> 4), j = 16 * (key_a & 0xFFFFFFFFll) + (rc & 15u);
    const long long k0 = 16 * (key_b >> 32), l0 = 16 * (key_b & 0xFFFFFFFFll);
    const long long k1 = k0 + 15 < mB ? k0 + 15 : mB - 1, l1 = l0 + 15 < nB ? l0 + 15 : nB - 1;
    const long long P0 = (i * mB + k0) >> 4, P1 = (i * mB + k1) >> 4, Q0 = (j * nB + l0) >> 4, Q1 = (j * nB + l1) >> 4;
    if (!coff) {
        cnt[x] = (int)((P1 - P0 + 1) * (Q1 - Q0 + 1));
        return;
    }
    uint64_t *out = keys + coff[x];
    for (long long P = P0; P <= P1; ++P)
        for (long long Q = Q0; Q <= Q1; ++Q) *out++ = ((uint64_t)P << bits_tc) | (uint64_t)Q;
}

// Row p of R in the tile column Q: the walk over the stored A(i, j) whose block reaches the tile and, for each, over B's row k there.
// Returns the row's 16-bit mask.  FILL: also writes the row's entries from slot e on, never at or past e_end.
template <bool FILL, typename VT>
__device__ __forceinline__ unsigned kr_walk(const TileSide &A, const TileSide &B, const long long p, const long long Q, const int r, const int op,
                                            const VT *__restrict__ a_vals, const VT *__restrict__ b_vals, int e, const int e0, const int e_end,
                                            const int tile, uint8_t *__restrict__ rowcolidx, int *__restrict__ headx, VT *__restrict__ vals)
{
    const unsigned mB = (unsigned)B.rows, nB = (unsigned)B.cols;
    const unsigned i = (unsigned)p / mB, k = (unsigned)p - i * mB;   // (p < rows of R <= INT32_MAX)
    const long long q0 = 16 * Q;
    const long long qn = (long long)A.cols * nB - 1;   // R's last column
    const long long q1 = q0 + 15 < qn ? q0 + 15 : qn;
    const int jlo = (int)((unsigned)q0 / nB), jhi = (int)((unsigned)q1 / nB);   // jhi - jlo <= 15, jhi < A.cols
    const int abase = jlo >> 4;
    const RowSeg sa = row_seg(A, (int)i, abase);
    unsigned rowmask = 0u;
    int bc = -1;
    RowSeg sb = {0u, 0u, 0u, 0, 0};
    for (int j = jlo; j <= jhi; ++j) {
        const unsigned ab = (unsigned)(j - 16 * abase);   // <= 15 + 15
        if (!((sa.m >> ab) & 1u)) continue;
        const long long off = (long long)j * nB - q0;   // where B's column 0 lands in the tile: -nB < off < 16
        const long long llo = off < 0 ? -off : 0;
        const long long lhi = 15 - off < (long long)nB - 1 ? 15 - off : (long long)nB - 1;   // llo <= lhi <= llo + 15
        const int c = (int)(llo >> 4);
        if (c != bc) {
            sb = row_seg(B, (int)k, c);
            bc = c;
        }
        const unsigned sh = (unsigned)(llo - 16 * (long long)c);           // B's column llo in the segment: 0 .. 15
        const unsigned width = (unsigned)(lhi - llo) + 1u;                 // 1 .. 16
        const unsigned bits = (sb.m >> sh) & ((1u << width) - 1u);         // bit b = B's column llo + b
        const unsigned place = (unsigned)(off + llo);                      // its column in the tile: 0 .. 15, place + width <= 16
        rowmask |= bits << place;
        if constexpr (FILL) {
            if (!bits) continue;
            const VT a = a_vals[seg_slot(sa, ab)];
            e = write_row_bits(bits, place, r, e, e0, e_end, tile, rowcolidx, headx, vals,
                               [&](const unsigned b) { return pem_binop_value<VT>(op, a, b_vals[seg_slot(sb, sh + b)]); });
        }
    }
    return rowmask;
}

// 16 lanes per candidate c, lane = local row r: rmask[16c + r] = the row's mask, cnt[c] = the tile's entries, flag[c] = it has any.
__global__ void __launch_bounds__(256) kr_count_kernel(const uint64_t *__restrict__ keys, long long ncand, TileSide A, TileSide B, long long r_rows,
                                                       int bits_tc, uint16_t *__restrict__ rmask, int *__restrict__ cnt, int *__restrict__ flag)
{
    const long long c = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int r = threadIdx.x & 15;
    unsigned m = 0u;
    if (c < ncand) {
        const CandKey k = cand_key(keys, c, bits_tc);
        const long long p = 16 * k.P + r;
        if (!k.dup && p < r_rows) m = kr_walk<false, float>(A, B, p, k.Q, r, 0, nullptr, nullptr, 0, 0, 0, 0, nullptr, nullptr, nullptr);
        rmask[16 * c + r] = (uint16_t)m;
    }
    cand_count(__popc(m), c, ncand, r, cnt, flag);
}

// 16 lanes per candidate, lane = local row r: the walk again, from the row's first slot
template <typename VT>
__global__ void __launch_bounds__(256) kr_fill_kernel(const uint64_t *__restrict__ keys, long long ncand, TileSide A, TileSide B, int bits_tc, int op,
                                                      const VT *__restrict__ a_vals, const VT *__restrict__ b_vals,
                                                      const uint16_t *__restrict__ rmask, const int *__restrict__ roff, const int *__restrict__ rid,
                                                      long long *__restrict__ tile_keys, int *__restrict__ tile_nnz_ptr,
                                                      uint8_t *__restrict__ rowcolidx, int *__restrict__ headx, VT *__restrict__ vals)
{
    const long long c = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int r = threadIdx.x & 15;
    const int n = c < ncand ? __popc((unsigned)rmask[16 * c + r]) : 0;
    cand_slots(c, ncand, r, n, roff, rid, tile_nnz_ptr, headx, [&](const CandSlots &s) {
        const CandKey k = cand_key(keys, c, bits_tc);
        cand_tile_head(r, s, k.P, k.Q, tile_keys, tile_nnz_ptr);
        if (!n) return;
        kr_walk<true, VT>(A, B, 16 * k.P + r, k.Q, r, op, a_vals, b_vals, s.e, s.e0, s.e1, s.t, rowcolidx, headx, vals);
    });
}

// the refresh map, once.  Entry (p, q) of R is A(p / mB, q / nB) op B(p % mB, q % nB): each operand's tile by mask_find_tile, its
// slot by src_slot.
__global__ void __launch_bounds__(256) kr_map_kernel(const long long *__restrict__ r_keys, long long nt, const int *__restrict__ r_ptr,
                                                     const uint8_t *__restrict__ r_rci, TileSide A, TileSide B, int2 *__restrict__ map)
{
    const unsigned mB = (unsigned)B.rows, nB = (unsigned)B.cols;
    for_tile_entries(r_keys, nt, r_ptr, r_rci, [&](const int e, const long long pl, const long long ql) {
        const unsigned p = (unsigned)pl, q = (unsigned)ql;   // (below R's rows and columns)
        const unsigned i = p / mB, k = p - i * mB, j = q / nB, l = q - j * nB;
        const int t_a = mask_find_tile(A.rowptr, A.colidx, (int)(i >> 4), (int)(j >> 4));
        const int t_b = mask_find_tile(B.rowptr, B.colidx, (int)(k >> 4), (int)(l >> 4));
        map[e] = make_int2(t_a >= 0 ? src_slot(A.ptr[t_a], A.rec[16 * (size_t)t_a + (i & 15u)], j & 15u) : 0,
                           t_b >= 0 ? src_slot(B.ptr[t_b], B.rec[16 * (size_t)t_b + (k & 15u)], l & 15u) : 0);
    });
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
// the arguments were checked (kron_sizes_ok): the dimensions and nnz(A) * nnz(B) fit an int32
template <typename VT>
static pem_status kron_build(pem_ctx *ctx, const pem_tiled *A, const pem_tiled *B, int op, pem_tiled *R, const char *fn)
{
    set_tiled_shape(R, A->value_bytes, A->rows * B->rows, A->cols * B->cols);
    Derivation &d = R->derived;
    d.kind = Derivation::KRON;
    d.src[0] = A->serial;
    d.src[1] = B->serial;
    d.op = op;
    PEM_TRY(zero_flags(ctx));
    const int bits_tc = bits_for((uint64_t)R->tile_cols);
    const size_t ta = (size_t)A->ntiles, tb = (size_t)B->ntiles;
    const size_t npairs = A->nnz && B->nnz ? (size_t)A->nnz * tb : 0;   // (<= nnz(A) * nnz(B))
    DevBuf coff;   // per (A entry, B tile): the R tiles it reaches -> where its keys start
    PEM_TRY(coff.reserve(sizeof(int) * (npairs + 4)));
    auto cand = [&](int *cnt, const int *off, uint64_t *keys) {   // the counts, then (with their scan) the keys
        PEM_LAUNCH(ctx, kr_cand_kernel, grid_for(npairs, 256), 256, A->tile_keys.as<long long>(), A->tile_nnz_ptr.as<int>(), (long long)ta,
                   A->rowcolidx.as<uint8_t>(), B->tile_keys.as<long long>(), (long long)tb, (long long)npairs, B->rows, B->cols, bits_tc, cnt, off, keys);
    };
    if (npairs) cand(coff.as<int>(), nullptr, nullptr);
    PEM_TRY(exclusive_scan_i32(ctx, coff.as<int>(), coff.as<int>(), npairs, ctx->d_scalars));
    int64_t tot[1] = {0};
    PEM_TRY(check_candidates(ctx, 1, tot, fn));
    const size_t ncand = (size_t)tot[0];

    DevBuf rmask;   // per candidate: its 16 row masks, from the count to the fill
    PEM_TRY(rmask.reserve(sizeof(uint16_t) * 16 * (ncand + 1)));
    const TileSide sa = tile_side(A), sb = tile_side(B);
    CandidateStages st;
    st.emit = [&](uint64_t *keys) { cand(nullptr, coff.as<int>(), keys); };
    st.count = [&](const uint64_t *keys, int *cnt, int *flag) {
        PEM_LAUNCH(ctx, kr_count_kernel, grid_for(16 * ncand, 256), 256, keys, (long long)ncand, sa, sb, (long long)R->rows, bits_tc,
                   rmask.as<uint16_t>(), cnt, flag);
    };
    st.fill = [&](const uint64_t *keys, const int *roff, const int *rid, int *headx) {
        PEM_LAUNCH(ctx, kr_fill_kernel<VT>, grid_for(16 * ncand, 256), 256, keys, (long long)ncand, sa, sb, bits_tc, op, A->vals.as<VT>(),
                   B->vals.as<VT>(), rmask.as<uint16_t>(), roff, rid, R->tile_keys.as<long long>(), R->tile_nnz_ptr.as<int>(),
                   R->rowcolidx.as<uint8_t>(), headx, R->vals.as<VT>());
    };
    // (every (A entry, B entry) pair is exactly one entry of R)
    return tiling_from_candidates(ctx, R, fn, ncand, true, A->nnz * B->nnz, "nnz(A) * nnz(B) =", st);
}

// everything the host knows, in 64 bits, before anything is launched or allocated
static pem_status kron_sizes_ok(const pem_tiled *A, const pem_tiled *B, const char *fn)
{
    const long long rows = (long long)A->rows * B->rows, cols = (long long)A->cols * B->cols;
    if (rows > 0x7FFFFFFFll || cols > 0x7FFFFFFFll) {
        set_error("%s: the result would be %lld x %lld; a dimension holds at most INT32_MAX", fn, rows, cols);
        return PEM_E_OVERFLOW;
    }
    // (nnz <= rows * cols < 2^62 each, but the product of two such may not fit 64 bits: compare by division)
    if (A->nnz && B->nnz && A->nnz > 0x7FFFFFFFll / B->nnz) {
        set_error("%s: the result's entries exceed the int32 index range", fn);
        return PEM_E_OVERFLOW;
    }
    return PEM_OK;
}

extern "C" pem_status pem_tiled_kron(pem_ctx *ctx, const pem_tiled *A, const pem_tiled *B, int op, pem_tiled **out)
{
    const char *fn = "pem_tiled_kron";
    if (out) *out = nullptr;
    if (!ctx || !A || !B || !out) {
        set_error("%s: null context, operand or output", fn);
        return PEM_E_INVALID;
    }
    if (op < PEM_BINOP_PLUS || op > PEM_BINOP_LAND) {
        set_error("%s: unknown op %d (PEM_BINOP_PLUS .. PEM_BINOP_LAND = 0 .. 5)", fn, op);
        return PEM_E_INVALID;
    }
    if (A->value_bytes != B->value_bytes) {
        set_error("%s: A holds %s values, B %s", fn, A->value_bytes == 4 ? "fp32" : "fp64", B->value_bytes == 4 ? "fp32" : "fp64");
        return PEM_E_INVALID;
    }
    PEM_TRY(kron_sizes_ok(A, B, fn));
    return build_derived(ctx, out, [&](pem_tiled *R) {
        pem_status s = A->value_bytes == 4 ? kron_build<float>(ctx, A, B, op, R, fn) : kron_build<double>(ctx, A, B, op, R, fn);
        (void)hipStreamSynchronize(ctx->stream);   // (the temporaries went back to the arena)
        return s;
    });
}

// once: every entry's slots in A's and in B's vals
static pem_status kron_map(pem_ctx *ctx, pem_tiled *t, const pem_tiled *A, const pem_tiled *B)
{
    const size_t nnz = (size_t)t->nnz, nt = (size_t)t->ntiles;
    PEM_TRY(t->derived.map.reserve(sizeof(int2) * (nnz + 1)));
    PEM_LAUNCH(ctx, kr_map_kernel, grid_for((nt + 63) / 64 * 64, 256), 256, t->tile_keys.as<long long>(), (long long)nt, t->tile_nnz_ptr.as<int>(),
               t->rowcolidx.as<uint8_t>(), tile_side(A), tile_side(B), t->derived.map.as<int2>());
    return PEM_OK;
}

extern "C" pem_status pem_tiled_set_values_from_kron(pem_ctx *ctx, pem_tiled *t, const pem_tiled *A, const pem_tiled *B)
{
    const char *fn = "pem_tiled_set_values_from_kron";
    if (!ctx || !t || !A || !B) {
        set_error("%s: null context, tiling or operand", fn);
        return PEM_E_INVALID;
    }
    if (t->derived.kind != Derivation::KRON || t->derived.src[0] != A->serial || t->derived.src[1] != B->serial) {
        set_error("%s: the tiling was not made by pem_tiled_kron from this A and this B (in this order)", fn);
        return PEM_E_INVALID;
    }
    return refresh_derived(
        ctx, t, [&] { return kron_map(ctx, t, A, B); }, [&] { refresh_pairs(ctx, t, A->vals.p, B->vals.p, t->derived.op); });
}
