// tiled_internal.h -- what the units that build or refresh a tiling share (convert.hip, values.hip, chain.hip).
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

}  // namespace pem
