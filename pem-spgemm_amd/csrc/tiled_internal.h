// tiled_internal.h -- what the units that build, refresh or look up a tiling share (convert.hip, values.hip, chain.hip, mask.hip,
// ewise.hip).
#pragma once
#include "pem_internal.h"

namespace pem {

// sizing phase "tiles" of a tiling whose rows, cols, nnz, ntiles and value_bytes are set: every per-tile array (and the
// nnz-sized payload) in one driver allocation
pem_status reserve_tile_arrays(pem_ctx *ctx, pem_tiled *T);
// everything that follows from the sorted tile payload (tile_keys, tile_nnz_ptr, rowcolidx, vals); headx[0..nnz] = exclusive
// scan of the tile-head flags.  ctx->ev[6] must have been recorded where the caller's payload kernels start.  Synchronises.
pem_status derive_tiled(pem_ctx *ctx, pem_tiled *T, const int *headx, int bits_tr, int bits_tc);
// vmap_t (every entry's slot in vals_t) on first use (values.hip)
pem_status ensure_vmap_t(pem_ctx *ctx, pem_tiled *T);

// ---- device: tile lookups in a tiling's tile CSR (mask.hip, ewise.hip) ----
// M's tile id at (i, j), -1 where M has none: binary search in M's tile row i (tile_colidx is sorted inside a row)
__device__ __forceinline__ int mask_find_tile(const int *__restrict__ m_rowptr, const int *__restrict__ m_colidx, const int i, const int j)
{
    int lo = m_rowptr[i];
    const int end = m_rowptr[i + 1];
    int hi = end;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (m_colidx[mid] < j)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < end && m_colidx[lo] == j ? lo : -1;
}

// the first tile of tile row i whose column is >= j (a global tile id; m_rowptr[i + 1] when there is none): where (i, j) is or
// would be in the sorted tile list
__device__ __forceinline__ int tile_lower_bound(const int *__restrict__ m_rowptr, const int *__restrict__ m_colidx, const int i, const int j)
{
    int lo = m_rowptr[i];
    int hi = m_rowptr[i + 1];
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (m_colidx[mid] < j)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

}  // namespace pem
