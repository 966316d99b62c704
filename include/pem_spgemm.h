/*
 * pem_spgemm.h -- C ABI of libpemspgemm_hip.so: the MI355X-native tiled SpGEMM hot path.
 *
 * The reference (stckvrflw/pem-spgemm) has no library boundary: `main()` launches its CUDA
 * kernels inline with raw device pointers (spgemm.cu:939-952, 1138-1336).  This header is
 * the boundary a maintainer would cut along those call sites; every entry point names the
 * reference lines it replaces.  Plain pointers and sizes only -- no C++/torch types.
 *
 * Conventions
 *   - every function returns pem_status (0 = ok, <0 = error); pem_last_error() gives the
 *     message of the calling thread's last failure.  The library never calls exit().
 *   - handles are opaque; the library owns all device memory behind them.  Host buffers
 *     passed in or out are caller-owned.  `*_device` variants take/return device pointers
 *     valid on the context's device and are ordered on the context's stream.
 *   - one context per GPU rank; a context is single-caller.  Distinct contexts are
 *     independent (thread-safe across contexts).
 *   - indices are int32 like the reference's (`int`), sizes crossing the ABI are int64.
 *   - tiles are 16x16, values are fp64 (spgemm.cu:727-728).
 */
#ifndef PEM_SPGEMM_H
#define PEM_SPGEMM_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int pem_status;
enum {
    PEM_OK = 0,
    PEM_E_INVALID = -1,     /* bad argument / shape mismatch / index out of range */
    PEM_E_DUPLICATE = -2,   /* duplicate (i,j) in the input (the reference mishandles these) */
    PEM_E_NOMEM = -3,       /* device or host allocation failed */
    PEM_E_OVERFLOW = -4,    /* a count does not fit the reference's int32 arrays */
    PEM_E_HIP = -5,         /* HIP runtime error */
    PEM_E_STATE = -6,       /* steps called out of order */
    PEM_E_NODEVICE = -7,    /* no usable GPU: the product path has no CPU fallback */
    PEM_E_IO = -8,          /* tiled-format cache: file missing, unreadable, truncated, corrupt or not a cache file */
    PEM_E_STALE = -9        /* tiled-format cache: the file is intact but was made from a different source */
};

typedef struct pem_ctx pem_ctx;
typedef struct pem_tiled pem_tiled;   /* one matrix in tiled-CSR form, usable as A or as B */
typedef struct pem_cplan pem_cplan;   /* C = A*B over a tile-row range of A: symbolic + numeric result */

const char *pem_last_error(void);
const char *pem_version(void);

/* ---- context ------------------------------------------------------------------------ */
/* Replaces the stream/event/pool set-up of spgemm.cu:730-758, 808-817.  `stream` is a
 * hipStream_t passed as void* (NULL: the context creates its own stream). */
pem_status pem_ctx_create(int device, pem_ctx **out);
pem_status pem_ctx_create_on_stream(int device, void *stream, pem_ctx **out);
pem_status pem_ctx_destroy(pem_ctx *ctx);
pem_status pem_ctx_synchronize(pem_ctx *ctx);

/* Device memory.  The reference sizes two rmm pools once (spgemm.cu:808-817) and takes the eleven per-iteration
 * buffers of its timed loop from a pool (cudaMallocAsync / cudaFreeAsync, spgemm.cu:1138-1295, 1118-1131).  Here every
 * context owns an arena: the driver is asked for memory in few large slabs, all buffers of the context's tilings, plans
 * and temporaries are carved out of them, and memory a destroyed handle gives back stays in the arena for the next one.
 * A pass on a new plan therefore makes at most one driver allocation per sizing phase (pairs / C tiles / C entries) and
 * none at all once the arena holds enough.  pem_ctx_reserve sizes the arena ahead of time (one driver allocation of
 * `bytes`, skipped if a free block that large exists); pem_ctx_trim returns wholly free slabs to the driver. */
pem_status pem_ctx_reserve(pem_ctx *ctx, int64_t bytes);
pem_status pem_ctx_trim(pem_ctx *ctx);
typedef struct {
    int64_t slab_bytes;         /* held from the driver                         */
    int64_t in_use_bytes;       /* handed out to live buffers                   */
    int64_t peak_in_use_bytes;
    int64_t largest_free_bytes; /* largest request served without the driver    */
    int64_t driver_allocs;      /* hipMalloc calls so far                       */
    int64_t block_allocs;       /* buffers carved so far                        */
} pem_memory_stats;
pem_status pem_ctx_memory_stats(pem_ctx *ctx, pem_memory_stats *out);

/* ---- a2-a7: COO / CSR -> tiled CSR ---------------------------------------------------- */
/* Replaces spgemm.cu:832-1066 (decide_which_tile, thrust sort/unique/reduce_by_key/scan,
 * COO->CSR, generate_tiles_csr, __transpose_B_mask, tile-level CSR/CSC + _B_tileOffsets).
 * transpose != 0 builds the tiling of M^T (spgemm.cu:788-792).  Every tiled matrix carries
 * both roles' metadata (A side: tile CSR; B side: transposed masks + tile CSC). */
pem_status pem_tiled_from_coo(pem_ctx *ctx, int rows, int cols, int64_t nnz, const int32_t *I,
                              const int32_t *J, const double *V, int transpose, pem_tiled **out);
pem_status pem_tiled_from_coo_device(pem_ctx *ctx, int rows, int cols, int64_t nnz, const int32_t *dI,
                                     const int32_t *dJ, const double *dV, int transpose, pem_tiled **out);
pem_status pem_tiled_from_csr(pem_ctx *ctx, int rows, int cols, const int32_t *rowptr,
                              const int32_t *colidx, const double *V, pem_tiled **out);
pem_status pem_tiled_destroy(pem_ctx *ctx, pem_tiled *t);

/* fp32 values.  The reference pins `ValueType = double` in main (spgemm.cu:728) although its kernels
 * are templates on it (spgemm.cu:137, 593).  The `_f32` entry points build a tiling whose values (and the values of
 * every C computed from it) are float: step 3 then runs one fmaf per product, in the same ascending-k order.  A and
 * B of one plan must share a value type; the fp64 export entry points refuse an fp32 plan and vice versa. */
pem_status pem_tiled_from_coo_f32(pem_ctx *ctx, int rows, int cols, int64_t nnz, const int32_t *I,
                                  const int32_t *J, const float *V, int transpose, pem_tiled **out);
pem_status pem_tiled_from_coo_device_f32(pem_ctx *ctx, int rows, int cols, int64_t nnz, const int32_t *dI,
                                         const int32_t *dJ, const float *dV, int transpose, pem_tiled **out);
pem_status pem_tiled_from_csr_f32(pem_ctx *ctx, int rows, int cols, const int32_t *rowptr,
                                  const int32_t *colidx, const float *V, pem_tiled **out);

typedef struct {
    int32_t rows, cols;            /* of the tiled matrix (after transpose)           */
    int64_t nnz;
    int32_t tile_rows, tile_cols;  /* ceil(rows/16), ceil(cols/16)  spgemm.cu:840-843 */
    int64_t ntiles;                /* non-empty 16x16 tiles         spgemm.cu:871     */
    double conv_ms;                /* device time of the whole conversion             */
    double conv_tile_kernel_ms;    /* tile payload kernels only (CSV cols 5/6, spgemm.cu:938-978) */
    int32_t value_bytes;           /* 8: fp64 (the reference's ValueType), 4: fp32    */
    int32_t reserved;
} pem_tiled_info;
pem_status pem_tiled_get_info(const pem_tiled *t, pem_tiled_info *info);

/* Stage-level views (D2H copy of one array; `bytes` must equal the array's size). */
typedef enum {
    PEM_T_TILE_KEYS = 0,     /* int64[T]   (tileRow<<32)|tileCol, sorted         spgemm.cu:131-133, 869-877 */
    PEM_T_TILE_NNZ_PTR,      /* int32[T+1] perTileNnz exclusive scan             spgemm.cu:873-874 */
    PEM_T_MASKS,             /* uint16[16T] row bitmasks                         spgemm.cu:196-200 */
    PEM_T_ROWPTR,            /* uint8[16T] nnz before row r inside the tile      spgemm.cu:205-209 */
    PEM_T_ROWCOLIDX,         /* uint8[nnz] (r<<4)|c                              spgemm.cu:195, 221 */
    PEM_T_VALS,              /* double[nnz] (float[nnz] for an fp32 tiling) tile order, row-major inside a tile  spgemm.cu:220 */
    PEM_T_MASKS_T,           /* uint16[16T] transposed masks                     spgemm.cu:244-253 */
    PEM_T_TILE_ROWPTR,       /* int32[tile_rows+1]                               spgemm.cu:986-999 */
    PEM_T_TILE_COLIDX,       /* int32[T]                                         spgemm.cu:1001-1006 */
    PEM_T_TILE_COLPTR,       /* int32[tile_cols+1]                               spgemm.cu:1042-1055 */
    PEM_T_TILE_ROWIDX,       /* int32[T]                                         spgemm.cu:1056-1061 */
    PEM_T_TILE_OFFSETS       /* int32[T] CSC position -> CSR tile id             spgemm.cu:1034-1040 */
} pem_tiled_array;
pem_status pem_tiled_get_array(pem_ctx *ctx, const pem_tiled *t, pem_tiled_array which, void *host_dst, int64_t bytes);

/* ---- on-disk cache of the tiled format -------------------------------------
 * The reference parses the .mtx text and re-runs the whole conversion on every start, and its conversion clock
 * includes the parse (spgemm.cu:760-1066).  A cache file holds the sorted tile payload of one tiling -- the tile
 * list (spgemm.cu:869-877), perTileNnz (873-874), rowColIdx (195, 221) and vals (220) -- little-endian, with a
 * checksum.  Loading uploads the four arrays, checks them ON THE DEVICE (sorted distinct in-range tiles, 1..256
 * entries per tile, strictly ascending (r<<4|c) inside a tile, every entry inside rows x cols), then rebuilds the
 * masks, intra-tile row pointers, transposed masks and the tile-level CSR/CSC indices with the conversion's own
 * kernels: no parse, no sort.  A file that fails any check is rejected, never half-used.
 * `key` identifies what the tiling was made from (the caller's choice, e.g. size + mtime of the .mtx and the
 * transpose flag); load with a non-NULL `expect` returns PEM_E_STALE when the stored key differs. */
typedef struct {
    uint64_t source_size;      /* bytes of the source file                  */
    int64_t source_mtime_ns;   /* its modification time                     */
    uint32_t transpose;        /* the tiling is of the transposed source    */
    uint32_t reserved;         /* 0                                         */
} pem_cache_key;
pem_status pem_tiled_save(pem_ctx *ctx, const pem_tiled *t, const char *path, const pem_cache_key *key);
pem_status pem_tiled_load(pem_ctx *ctx, const char *path, const pem_cache_key *expect, pem_tiled **out);

/* ---- numeric refresh (new; the reference re-runs its whole loop) ----------------------------
 * Replaces the values of a tiling in place; its structure, and every plan's steps 1-2 built on it, stay valid.  V holds
 * exactly nnz values in one of two orders of the TILED matrix (after any transpose at conversion):
 *   PEM_VALUES_ROW_MAJOR: by (row, col) ascending -- the order of a CSR with sorted columns (scipy canonical form);
 *   PEM_VALUES_COL_MAJOR: by (col, row) ascending -- for a tiling built with transpose = 1 this is the source matrix's CSR
 *                         order, i.e. the caller passes the same array to A and to its A^T tiling.
 * The order is a property of the tiled arrays, not of the input the tiling came from: any tiling works, also one made by
 * pem_tiled_load.  Values are copied bit for bit (NaN payloads, -0.0, inf and subnormals arrive unchanged).
 *
 * The numeric-only product is the existing pem_spgemm_step3: after steps 1 and 2 have run on a plan, set_values on its A
 * and/or B followed by pem_spgemm_step3 recomputes C from the new values.  pem_spgemm on such a plan does the same (its
 * repeat pass re-runs steps 1-2 on the unchanged structure).
 *
 * Host forms upload the values, refresh them and wait.  `_device` forms take a device array, are ordered on the context's
 * stream and return without waiting or reading anything back; a kernel failure surfaces at pem_ctx_synchronize, as for
 * pem_c_export_csr_device.  PEM_E_INVALID for a null context or tiling, a null V with nnz > 0, an order that is not 0 or 1,
 * or a value type that does not match the tiling (the rule of the export entry points).  A tiling with nnz = 0: no-op, PEM_OK.
 *
 * The first refresh in an order builds that order's map (int32 per entry, the position of every entry's value in V) and, on
 * the tiling's first refresh, the map of its vals_t slots: 4 bytes per entry each, carved from the context's arena and kept
 * with the tiling.  Later refreshes are one kernel that gathers V into vals and vals_t.
 *
 * Staleness.  Every tiling carries a value version, bumped by each refresh; a plan records its A's and B's versions when
 * pem_spgemm or pem_spgemm_step3 completes.  While either operand has been refreshed since, the pem_c_export_* entry points
 * and pem_cplan_get_array(PEM_C_VALS) return PEM_E_STATE; the symbolic arrays (pairs, masks, offsets) stay readable.
 * pem_spgemm_step3 (or pem_spgemm) makes C current again.
 *
 * Graph replay (pem_set_graph_replay).  vals and vals_t are rewritten in place, never reallocated, so a graph pem_spgemm
 * captured earlier stays valid and reads the new values on its next replay.  Buffers a refresh allocates the first time (the
 * maps; the host forms' staging buffer when it has to grow) come from the arena, and the arena generation that bumps makes
 * such a graph re-capture once. */
typedef enum { PEM_VALUES_ROW_MAJOR = 0, PEM_VALUES_COL_MAJOR = 1 } pem_values_order;
pem_status pem_tiled_set_values(pem_ctx *ctx, pem_tiled *t, const double *V, int order);
pem_status pem_tiled_set_values_device(pem_ctx *ctx, pem_tiled *t, const double *dV, int order);
pem_status pem_tiled_set_values_f32(pem_ctx *ctx, pem_tiled *t, const float *V, int order);
pem_status pem_tiled_set_values_device_f32(pem_ctx *ctx, pem_tiled *t, const float *dV, int order);

/* ---- a8: flop count (spgemm.cu:1068-1079), computed on the device ------------------------ */
pem_status pem_flop_count(pem_ctx *ctx, const pem_tiled *A, const pem_tiled *B, uint64_t *flop);

/* ---- a9-a13: the three steps ---------------------------------------------------------- */
/* A plan covers tile rows [tile_row_begin, tile_row_end) of A (tile_row_end < 0: all); the
 * multi-GPU row-block split gives each rank one plan over its own range, B replicated. */
pem_status pem_cplan_create(pem_ctx *ctx, const pem_tiled *A, const pem_tiled *B,
                            int32_t tile_row_begin, int32_t tile_row_end, pem_cplan **out);
pem_status pem_cplan_destroy(pem_ctx *ctx, pem_cplan *plan);

/* Masked product C<M> = A*B (the GraphBLAS mxm with a structural mask): only the entries of A*B at the stored positions of M
 * (explicit zeros included; M's values are never read) -- or, with PEM_MASK_COMPLEMENT, only those where M stores nothing.
 * M is any tiling of the shape of C, A.rows x B.cols, fp32 or fp64 whatever the type of A and B; it may be A or B itself, and
 * it must outlive the plan.  The pattern of C is that of the unmasked plan (the symbolic product, entries that cancel
 * numerically included) intersected with M's (or with its complement); every kept value equals the unmasked product's at the
 * same position bit for bit.  pem_cplan_get_info and every pem_cplan_array describe C<M> (npairs_all stays the unmasked P; C
 * tiles the mask empties may remain in the tile list).  A tile-row range uses M's tile rows of the same (global) indices.
 * Masked plans always run the row-local step 1 and the fused step 2: setting PEM_OPT_STEP1_GLOBAL_SORT = 1 or PEM_OPT_WIDE = 0
 * on one returns PEM_E_INVALID.  M null, other flags or another shape: PEM_E_INVALID. */
typedef enum { PEM_MASK_STRUCTURE = 0, PEM_MASK_COMPLEMENT = 1 } pem_mask_flags;
pem_status pem_cplan_create_masked(pem_ctx *ctx, const pem_tiled *A, const pem_tiled *B, const pem_tiled *M, int mask_flags,
                                   int32_t tile_row_begin, int32_t tile_row_end, pem_cplan **out);

/* Semirings.  Step 3 reduces the products of every C entry (i, j) -- all k where A(i,k) and B(k,j)
 * are stored -- under the plan's semiring; the structure of C never depends on it (C stores exactly the entries the plus-times
 * plan stores, masked or not: the symbolic product), only the value at each entry does.
 *   PEM_SEMIRING_PLUS_TIMES (default)  the fma chain of every other entry point, bit for bit
 *   PEM_SEMIRING_MIN_PLUS              fmin over the products of (a + b), starting from +inf
 *   PEM_SEMIRING_MAX_PLUS              fmax over the products of (a + b), starting from -inf
 *   PEM_SEMIRING_MAX_TIMES             fmax over the products of (a * b), starting from -inf
 *   PEM_SEMIRING_PLUS_PAIR             the number of products, as a value of C's type (A's and B's values are never read)
 *   PEM_SEMIRING_LOR_LAND              1 if some product has a != 0 and b != 0 (NaN counts as != 0), else 0
 * Each a + b and a * b is rounded once in C's type, to nearest; the min/max semirings involve no fma.  min and max follow C's
 * fmin / fmax: a NaN product is skipped, an entry whose every product is NaN keeps the start value, and the sign of a zero result
 * is not specified.  Min/max results therefore do not depend on the order of the products.  plus_pair counts exactly up to 2^53
 * (fp64) / 2^24 (fp32).  lor_land stores 0.0 where every product has a zero operand: the entry stays, as plus-times keeps entries
 * that cancel.
 * pem_cplan_set_semiring is allowed at any time, on every plan (masked or not, fp64 or fp32, any option); setting the current
 * semiring is a no-op.  Changing it makes C's values stale, as a numeric refresh does: the pem_c_export_* entry points and
 * pem_cplan_get_array(PEM_C_VALS) return PEM_E_STATE until pem_spgemm_step3 or pem_spgemm runs again (the symbolic arrays stay
 * readable).  The intended use: one symbolic pass, then set_semiring + pem_spgemm_step3 per semiring.  A graph captured under
 * the old semiring (pem_set_graph_replay) is dropped; the next pem_spgemm captures again.  An unknown value or a null plan:
 * PEM_E_INVALID.  The pem_mgpu_* entry points always multiply under plus-times. */
typedef enum {
    PEM_SEMIRING_PLUS_TIMES = 0,
    PEM_SEMIRING_MIN_PLUS = 1,
    PEM_SEMIRING_MAX_PLUS = 2,
    PEM_SEMIRING_MAX_TIMES = 3,
    PEM_SEMIRING_PLUS_PAIR = 4,
    PEM_SEMIRING_LOR_LAND = 5
} pem_semiring;
pem_status pem_cplan_set_semiring(pem_cplan *plan, int semiring);
pem_status pem_cplan_get_semiring(const pem_cplan *plan, int *semiring);

/* Chained products: the C of a plan as the operand of the next product, built on the device from the
 * plan's tiled result -- no export, no host round trip, no entry-level sort.
 *   pem_tiled_from_cplan  a new tiling of C (transpose = 0: A.rows x B.cols) or of C^T (transpose = 1: B.cols x A.rows).  The shape
 *       is the full one also for a plan over a tile-row range: the tile rows outside the range are empty (for C^T, those tile
 *       columns), so a row block stays a row block under right multiplication.  The tiling holds exactly the stored entries of C
 *       (the symbolic product, entries that cancel included, as the exports); values are copied bit for bit in C's value type.  It
 *       equals, array for array, the tiling pem_tiled_from_csr builds from pem_c_export_csr of the same plan (with transpose = 1:
 *       pem_tiled_from_coo(..., transpose = 1) of the exported COO); C tiles without entries (PEM_OPT_PRUNE = 0, masked plans) are
 *       dropped.  The plan must have completed step 3 with current values (the rule of the exports): PEM_E_STATE before step 3,
 *       after a refresh of A or B or after pem_cplan_set_semiring.  A null argument or transpose not 0/1: PEM_E_INVALID.  An empty
 *       C gives a valid tiling with nnz = 0.  The tiling owns its arrays: the plan may be destroyed, re-run or re-optioned after.
 *       It works everywhere a tiling does (A, B, mask, save / load, set_values*, flop count, split).
 *   pem_tiled_set_values_from_cplan  the plan's current C values into such a tiling's vals and vals_t, in place; bumps its value
 *       version (plans built on it turn stale under the rule of pem_tiled_set_values until their step 3 runs).  Stream-ordered, never
 *       waits, reads nothing back.  PEM_E_INVALID if t was not made from this plan (every plan carries a process-wide serial the
 *       tiling records) or the plan's nnz differs from t's; PEM_E_STATE if the plan's C is not current.  C's value order does not
 *       depend on the plan's options or semiring, so the refresh stays valid after pem_cplan_set_option / set_semiring once step 3
 *       has run again.  A C^T tiling builds an int32 map per entry on its first refresh (4 bytes per entry, kept with the tiling);
 *       that and the vals_t map of pem_tiled_set_values are arena allocations, which make a captured graph re-capture once. */
pem_status pem_tiled_from_cplan(pem_ctx *ctx, const pem_cplan *plan, int transpose, pem_tiled **out);
pem_status pem_tiled_set_values_from_cplan(pem_ctx *ctx, pem_tiled *t, const pem_cplan *plan);

/* Element-wise combination of two tilings: with pem_tiled_from_cplan, C = alpha*A*B + beta*D and its
 * semiring forms stay on the device.
 *   pem_tiled_ewise  a new tiling R of A's shape and value type, owning its arrays, from A and B.  A and B must have the same rows x
 *       cols and value type; they may be the same handle, and either may be a tiling built with transpose = 1 (it is the tiling of its
 *       own matrix).  R works everywhere a tiling does (A, B, mask, save / load, set_values*, flop count, split).
 *     Pattern.  PEM_EWISE_UNION: every position stored in A or in B.  PEM_EWISE_INTERSECT: every position stored in both.  Explicit
 *       zeros and results that come out as 0 stay entries (the rule of sections 3f / 3g); tiles an intersection leaves without entries
 *       are not in R (1..256 entries per tile).
 *     Values, in the value type T, no fma and no wider intermediate.  a' = a if alpha == 1, else (T)alpha * a rounded once; b' from
 *       beta alike (alpha = beta = 1 copies the values bit for bit).  Where both are stored: op(a', b') --
 *         PEM_BINOP_PLUS a' + b', PEM_BINOP_TIMES a' * b' (each rounded once);
 *         PEM_BINOP_MIN / PEM_BINOP_MAX: C's fmin / fmax (a NaN side is skipped; the sign of a zero result is not specified);
 *         PEM_BINOP_LOR: 1 if a' != 0 || b' != 0, else 0;  PEM_BINOP_LAND: 1 if a' != 0 && b' != 0, else 0  (NaN counts as != 0).
 *       Where only one is stored (UNION only): a' or b' unchanged, whatever the op (GraphBLAS eWiseAdd).  A NaN that arithmetic
 *       produces has an unspecified payload.
 *     PEM_E_INVALID: a null argument, an unknown pattern or op, different shapes or different value types.  Empty operands or an empty
 *       intersection give a valid tiling with nnz = 0.  A's and B's values are read as they are when the call is made (stream order);
 *       the call waits, like pem_tiled_from_cplan, and its allocations come from the context's arena (a captured graph re-captures).
 *       Besides the tiling's own arrays R keeps 8 bytes per tile of R (the A and B tiles each of its tiles comes from) for the refresh.
 *   pem_tiled_set_values_from_ewise  recomputes t's values (vals and vals_t) in place from the current values of A and B, as
 *       pem_tiled_ewise would, and bumps t's value version.  Stream-ordered, never waits, reads nothing back; only the first call
 *       allocates (an int32 pair per entry: where its operand values sit in A and B).  PEM_E_INVALID unless t was made by
 *       pem_tiled_ewise from exactly this A and this B in this order: every tiling carries a process-wide serial, and t records both
 *       operands' (swapped operands, or a tiling recreated at a reused address, are refused). */
typedef enum { PEM_EWISE_UNION = 0, PEM_EWISE_INTERSECT = 1 } pem_ewise_pattern;
typedef enum {
    PEM_BINOP_PLUS = 0,
    PEM_BINOP_TIMES = 1,
    PEM_BINOP_MIN = 2,
    PEM_BINOP_MAX = 3,
    PEM_BINOP_LOR = 4,
    PEM_BINOP_LAND = 5
} pem_binop;
pem_status pem_tiled_ewise(pem_ctx *ctx, const pem_tiled *A, const pem_tiled *B, int pattern, int op, double alpha, double beta,
                           pem_tiled **out);
pem_status pem_tiled_set_values_from_ewise(pem_ctx *ctx, pem_tiled *t, const pem_tiled *A, const pem_tiled *B);

/* Select (GraphBLAS GrB_select): the stored entries of a tiling that satisfy a predicate, on the device.
 *   pem_tiled_select  a new tiling R of A's shape and value type, owning its arrays, holding exactly the stored entries of A that
 *       satisfy op with the thunk; values are copied bit for bit.  R works everywhere a tiling does (A, B, mask, save / load,
 *       set_values*, flop count, split, ewise, export, select).  Tiles left without entries are not in R (1..256 entries per tile);
 *       if nothing is kept, R is a valid tiling with nnz = 0.
 *     Coordinates.  (i, j) are those of the matrix the tiling represents (the matrix pem_tiled_export_csr returns): a tiling built
 *       with transpose = 1 is filtered as M^T.
 *     Positional ops (PEM_SELECT_TRIL .. PEM_SELECT_COL_GT) read no values.  The thunk is an integer k: it must be integral with
 *       |k| <= 2^31, else PEM_E_INVALID.  A k beyond the shape is legal and keeps everything or nothing.
 *     Value ops compare the value x with y = the thunk rounded once to the tiling's value type ((float)thunk, to nearest, for fp32),
 *       with IEEE comparisons in that type: -0.0 == 0.0; a NaN x fails every predicate but PEM_SELECT_VALUE_NE, and ABS_GT drops it;
 *       a NaN thunk is allowed (VALUE_NE keeps everything, the other value ops nothing).  VALUE_NE with thunk 0 drops explicit zeros.
 *     R equals the tiling pem_tiled_from_csr builds from the filtered pem_tiled_export_csr of A (every pem_tiled_info field but the
 *       two timings, every pem_tiled_array).  PEM_E_INVALID: a null argument, an unknown op, a bad positional thunk.  A's values are
 *       read as they are when the call is made (stream order); the call waits, and its allocations come from the context's arena (a
 *       captured graph re-captures once).  Besides the tiling's own arrays R keeps 4 bytes per tile of R (its tile in A).
 *   pem_tiled_set_values_from_select  positional ops only (their pattern does not depend on the values): rewrites t's vals and vals_t
 *       in place from A's current values and bumps t's value version.  Stream-ordered, never waits, reads nothing back; only the
 *       first call allocates (an int32 per entry: the slot of its value in A's vals).  PEM_E_INVALID unless t was made by
 *       pem_tiled_select from exactly this A (the serial rule of pem_tiled_set_values_from_ewise), and for a t made by a value op:
 *       its pattern depends on the values, so select again. */
typedef enum {
    /* position of entry (i, j) of the tiled matrix; k = thunk, an integer */
    PEM_SELECT_TRIL = 0,     /* j <= i + k */
    PEM_SELECT_TRIU = 1,     /* j >= i + k */
    PEM_SELECT_DIAG = 2,     /* j == i + k */
    PEM_SELECT_OFFDIAG = 3,  /* j != i + k */
    PEM_SELECT_ROW_LE = 4,   /* i <= k */
    PEM_SELECT_ROW_GT = 5,   /* i >  k */
    PEM_SELECT_COL_LE = 6,   /* j <= k */
    PEM_SELECT_COL_GT = 7,   /* j >  k */
    /* value x of the entry; y = thunk rounded once to the tiling's value type */
    PEM_SELECT_VALUE_EQ = 8, PEM_SELECT_VALUE_NE = 9, PEM_SELECT_VALUE_LT = 10,
    PEM_SELECT_VALUE_LE = 11, PEM_SELECT_VALUE_GT = 12, PEM_SELECT_VALUE_GE = 13,
    PEM_SELECT_ABS_GT = 14   /* fabs(x) > y: drop tolerance */
} pem_select_op;
pem_status pem_tiled_select(pem_ctx *ctx, const pem_tiled *A, int op, double thunk, pem_tiled **out);
pem_status pem_tiled_set_values_from_select(pem_ctx *ctx, pem_tiled *t, const pem_tiled *A);

/* Select top-k: the first k entries of every row or column of a tiling in rank order, on the device.
 *   pem_tiled_select_topk  a new tiling R of A's shape and value type, owning its arrays, holding of every line of A the first
 *       min(k, entries of the line) entries in the line's rank order and nothing else; values are copied bit for bit.  dim is a
 *       pem_reduce_dim: PEM_REDUCE_ROWS, a line is a matrix row and the index inside it is the column; PEM_REDUCE_COLS, a line is a
 *       matrix column and the index inside it is the row.  Untyped, like pem_tiled_select: one entry point serves fp64 and fp32.
 *     Rank order of a line.
 *       1. Entries whose value is not a NaN come before entries whose value is a NaN, under all three orders.
 *       2. Among numbers, PEM_TOPK_LARGEST ranks by x descending, PEM_TOPK_SMALLEST by x ascending, PEM_TOPK_ABS_LARGEST by |x|
 *          descending.  Comparisons are IEEE in the tiling's value type: -0.0 and 0.0 are equal, subnormals are compared as they
 *          are (no flush), +-inf are ordinary extremes.
 *       3. Equal entries, and NaNs among themselves, rank by ascending index inside the line: the lower column for rows, the lower
 *          row for columns.
 *       This is a total order, so the result is unique: every line of R has exactly min(k, n_line) entries, two calls give identical
 *       arrays, no NaN is kept while a number of the same line is dropped, and a NaN is kept only to fill a line that has fewer
 *       than k numbers.
 *     Coordinates are those of the matrix the tiling represents (the matrix pem_tiled_export_csr returns): a tiling built with
 *       transpose = 1 is its own matrix.
 *     k = 0 gives a valid tiling with nnz = 0; k at or above the longest line gives A's arrays again; an empty A gives an empty R.
 *       Tiles left without entries are not in R.  R equals the tiling pem_tiled_from_coo builds from the kept triples (every
 *       pem_tiled_info field but the two timings, every pem_tiled_array) and works everywhere a tiling does.
 *     PEM_E_INVALID, before anything is launched or allocated (*out stays NULL): a null context, A or out; an unknown order or dim;
 *       k < 0.  A's values are read as they are when the call is made (stream order); the call waits, and its allocations come from
 *       the context's arena.  With dim = PEM_REDUCE_COLS the first call on a tiling may build the column schedule of pem_tiled_mxv,
 *       which stays with the tiling.
 *     No refresh: the pattern depends on the values, so select again; pem_tiled_set_values_from_select refuses R. */
typedef enum { PEM_TOPK_LARGEST = 0, PEM_TOPK_SMALLEST = 1, PEM_TOPK_ABS_LARGEST = 2 } pem_topk_order;
pem_status pem_tiled_select_topk(pem_ctx *ctx, const pem_tiled *A, int order, int dim, int64_t k, pem_tiled **out);

/* Extract and transpose (GraphBLAS GrB_extract / GrB_transpose): the operations that re-index a tiling, on
 * the device.  None is typed: values are only copied, so one entry point serves fp64 and fp32 tilings, as pem_tiled_select does.
 *   pem_tiled_extract  a new tiling R = A(I, J) of ni x nj and A's value type, owning its arrays: R stores (p, q) exactly where A
 *       stores (I[p], J[q]), with that value copied bit for bit (explicit zeros stay; NaN payloads, -0.0, infinities and subnormals
 *       arrive unchanged).  I and J are host arrays; they may be in any order and may repeat indices (scipy's A[I][:, J]).
 *       I == NULL means all rows in order: ni is then ignored and R has A.rows rows.  J likewise.  A submatrix, a row or column
 *       sample, a symmetric permutation P*A*P^T (I = J = p) are all this call.
 *     Coordinates are those of the matrix the tiling represents (the matrix pem_tiled_export_csr returns): a tiling built with
 *       transpose = 1 is its own matrix.
 *     R equals the tiling pem_tiled_from_csr builds from the extracted matrix (every pem_tiled_info field but the two timings, every
 *       pem_tiled_array).  Tiles left without entries are not in R; if nothing is stored, R is a valid tiling with nnz = 0.  R works
 *       everywhere a tiling does (A, B, mask, save / load, set_values*, flop count, split, ewise, select, mxv, spmm, sddmm, export,
 *       extract, transpose).
 *     Refusals, all checked before anything is returned (*out stays NULL).  PEM_E_INVALID: a null context, tiling or out; a non-null
 *       list with n < 1 or n > INT32_MAX; an index < 0 or >= the dimension.  PEM_E_OVERFLOW: the result's entries or tiles exceed
 *       the int32 index range (repeated indices multiply entries); it is found by the counting pass, before the result is allocated.
 *     A's values are read as they are when the call is made (stream order); the call waits, and its allocations come from the
 *       context's arena (a captured graph re-captures once).  Besides the tiling's own arrays R keeps device copies of I and J for
 *       the refresh: 4 * (ni + nj) bytes (nothing for a null list).
 *   pem_tiled_extract_device  the same with dI, dJ in device memory on the context's device, read in stream order (they may be
 *       changed or freed once the call returns).  The indices are checked by the call's first kernel; a bad index is never used as
 *       an address.
 *   pem_tiled_set_values_from_extract  rewrites t's vals and vals_t in place from A's current values and bumps t's value version (the
 *       pattern of an extract does not depend on A's values, so every extract is refreshable).  Stream-ordered, never waits, reads
 *       nothing back; only the first call allocates (an int32 per entry: the slot of its value in A's vals).  PEM_E_INVALID unless t
 *       was made by pem_tiled_extract / pem_tiled_extract_device from exactly this A (the serial rule of
 *       pem_tiled_set_values_from_ewise).
 *   pem_tiled_transpose  a new tiling R = A^T of A.cols x A.rows, owning its arrays: array for array the tiling
 *       pem_tiled_from_coo(.., transpose = 1) builds from A's exported entries.  Any tiling works as A (converted, loaded, from_cplan,
 *       ewise, select, sddmm, extract).  PEM_E_INVALID: a null argument.  Waits; arena allocations, as above.
 *   pem_tiled_set_values_from_transpose  as pem_tiled_set_values_from_extract, for a t made by pem_tiled_transpose from exactly this A. */
pem_status pem_tiled_transpose(pem_ctx *ctx, const pem_tiled *A, pem_tiled **out);
pem_status pem_tiled_set_values_from_transpose(pem_ctx *ctx, pem_tiled *t, const pem_tiled *A);
pem_status pem_tiled_extract(pem_ctx *ctx, const pem_tiled *A, const int32_t *I, int64_t ni, const int32_t *J, int64_t nj, pem_tiled **out);
pem_status pem_tiled_extract_device(pem_ctx *ctx, const pem_tiled *A, const int32_t *dI, int64_t ni, const int32_t *dJ, int64_t nj,
                                    pem_tiled **out);
pem_status pem_tiled_set_values_from_extract(pem_ctx *ctx, pem_tiled *t, const pem_tiled *A);

/* Assign (GraphBLAS GrB_assign with no mask and no replace): writing a submatrix back, on the device -- the
 * dual of pem_tiled_extract.  None is typed: values are copied or combined in the tiling's own type, so one entry point serves fp64
 * and fp32 tilings.
 *   pem_tiled_assign  a new tiling Z of C's shape and value type, owning its arrays: C with Z(I, J) = A (accum = PEM_ACCUM_NONE) or
 *       Z(I, J) = op(C(I, J), A) (accum = a pem_binop).  C and A are not changed.  I holds ni row indices of C and J nj column indices
 *       of C, host arrays in any order that must not repeat an index (GraphBLAS leaves repeats undefined; they are refused here).
 *       I == NULL means all rows in order: ni is then ignored.  J likewise.  A is ni x nj (with a null I, A.rows == C.rows; J alike).
 *       C and A may be the same handle where the shapes allow it.
 *     Coordinates are those of the matrix the tiling represents (the matrix pem_tiled_export_csr returns).
 *     Outside I x J, Z stores what C stores, bit for bit.
 *     Inside, without an accum: Z stores (I[p], J[q]) exactly where A stores (p, q), with A's value bit for bit; C's entries in the
 *       region that A does not store are deleted, so assigning an empty ni x nj tiling clears the region.
 *     Inside, with an accum: Z stores the entry where C or A stores it; where both do, the value is op(c, a) under pem_tiled_ewise's
 *       arithmetic with alpha = beta = 1 (one rounding in the value type, fmin / fmax NaN rules, LOR / LAND giving 1.0 / 0.0); where
 *       only one does, that one's value unchanged.
 *     Explicit zeros and results that come out as 0 stay entries.  Tiles left without entries are not in Z; if nothing is stored, Z is
 *       a valid tiling with nnz = 0.  Z equals the tiling pem_tiled_from_coo builds from the assigned matrix (every pem_tiled_info field
 *       but the two timings, every pem_tiled_array) and works everywhere a tiling does (A, B, mask, save / load, set_values*, ewise,
 *       select, extract, transpose, mxv, spmm, sddmm, export, assign).
 *     Refusals, all checked before anything is returned (*out stays NULL, no handle changes).  PEM_E_INVALID: a null context, C, A or
 *       out; an unknown accum; different value types; a non-null list with n < 1 or n > INT32_MAX; an index < 0 or >= C's dimension;
 *       a repeated index; A's shape not ni x nj.  PEM_E_OVERFLOW: Z's entries or tiles exceed the int32 index range (with an accum
 *       only); it is found by a counting pass, before Z's payload is allocated.
 *     C's and A's values are read as they are when the call is made (stream order); the call waits, and its allocations come from the
 *       context's arena (a captured graph re-captures once); every intermediate is back in the arena when it returns.  Besides the
 *       tiling's own arrays Z keeps the inverses of the lists for the refresh: 4 * (C.rows + C.cols) bytes (nothing for a null list).
 *   pem_tiled_assign_device  the same with dI, dJ in device memory on the context's device, read in stream order (they may be changed
 *       or freed once the call returns).  Range and repeats are checked by the call's first kernel; a bad index is never used as an
 *       address.
 *   pem_tiled_set_values_from_assign  rewrites t's vals and vals_t in place from the current values of C and A, recomputing op(c, a)
 *       where both feed an entry, and bumps t's value version (the pattern of an assign does not depend on any value, so every assign
 *       is refreshable).  Stream-ordered, never waits, reads nothing back; only the first call allocates (an int32 pair per entry:
 *       its slots in C's and A's vals, -1 for none).  PEM_E_INVALID unless t was made by pem_tiled_assign / pem_tiled_assign_device
 *       from exactly this C and this A in this order (the serial rule of pem_tiled_set_values_from_ewise). */
enum { PEM_ACCUM_NONE = -1 };   /* otherwise a pem_binop */
pem_status pem_tiled_assign(pem_ctx *ctx, const pem_tiled *C, const pem_tiled *A, const int32_t *I, int64_t ni, const int32_t *J, int64_t nj,
                            int accum, pem_tiled **out);
pem_status pem_tiled_assign_device(pem_ctx *ctx, const pem_tiled *C, const pem_tiled *A, const int32_t *dI, int64_t ni, const int32_t *dJ,
                                   int64_t nj, int accum, pem_tiled **out);
pem_status pem_tiled_set_values_from_assign(pem_ctx *ctx, pem_tiled *t, const pem_tiled *C, const pem_tiled *A);

/* Apply and scale (GraphBLAS GrB_apply and the diagonal products D*A, A*D): new values on an unchanged
 * pattern, on the device.
 *   pem_tiled_apply  a new tiling R of A's shape and value type, owning its arrays, that stores exactly the positions A stores with
 *       the value f(x) of A's value x; f is op, for the binary ops bound to y = the thunk rounded once to the tiling's value type
 *       ((float)thunk, to nearest, for fp32).
 *   pem_tiled_scale  the same with z_ij = op(op(r_i, a_ij), c_j), evaluated left to right, op a pem_binop: PLUS, TIMES, MIN, MAX, LOR
 *       and LAND under pem_tiled_ewise's arithmetic with alpha = beta = 1 (LOR / LAND give 1.0 / 0.0, NaN counts as != 0).  d_row holds
 *       A.rows and d_col A.cols values of the tiling's value type, device arrays on the context's device (pem_tiled_scale for fp64
 *       tilings, pem_tiled_scale_f32 for fp32 ones).  A null vector means that step is not performed at all (not "times 1"): with
 *       both null R's values are A's bit for bit.  TIMES is D_r * A * D_c; PLUS is a_ij + h_i + g_j, the reweighting in front of
 *       min_plus / max_plus products.  The vectors are read only at the indices of stored entries, never past rows - 1 / cols - 1.
 *     Pattern.  Explicit zeros stay entries, and so do results that come out as 0, inf or NaN (the rule of pem_tiled_ewise and
 *       pem_tiled_select): nothing is ever dropped.  An empty A gives a valid tiling with nnz = 0.  R equals the tiling
 *       pem_tiled_from_coo builds from A's exported entries with the transformed values (every pem_tiled_info field but the two
 *       timings, every pem_tiled_array) and works everywhere a tiling does (A, B, mask, save / load, set_values*, ewise, select,
 *       extract, transpose, assign, mxv, spmm, sddmm, export, apply, scale).  Any tiling works as A.
 *     Coordinates are those of the matrix the tiling represents (the matrix pem_tiled_export_csr returns): a tiling built with
 *       transpose = 1 is its own matrix.
 *     Arithmetic.  Everything is computed in the value type with one rounding per operation: no fma, no wider intermediate.  1 / x,
 *       x / y and sqrt are IEEE correctly rounded in fp64 and fp32, subnormals kept.  MIN / MAX are C's fmin / fmax (a NaN side is
 *       skipped; the sign of a zero result is not specified).  A NaN that arithmetic produces has an unspecified payload; IDENTITY,
 *       ABS and AINV only touch the sign bit and keep payloads.  POWI: with the bits of k = 1 b_(m-1) .. b_0, p = x, then for b from
 *       b_(m-1) down to b_0: p = p * p, and p = p * x if b is set; each product rounded once, so k = 1 copies x bit for bit and
 *       k = 2 is x * x.  General pow, exp and log are not offered: no device implementation of them is correctly rounded.
 *     Refusals, all checked before anything is returned (*out stays NULL, no handle changes).  PEM_E_INVALID: a null context, A or
 *       out; an unknown op; a POWI thunk that is not an integer in 1 .. 64; the fp64 form of scale on an fp32 tiling or the reverse.
 *       A NaN thunk is allowed, as in pem_tiled_select, and simply propagates.
 *     A's values and the vectors are read as they are when the call is made (stream order); the call waits, and its allocations come
 *       from the context's arena (a captured graph re-captures once).  R's structural arrays are device copies of A's.  Besides the
 *       tiling's own arrays a scale result keeps an int32 per entry (its slot in vals_t) for its refresh.
 *   pem_tiled_set_values_from_apply  recomputes t's vals and vals_t in place from A's current values with the op and thunk t was made
 *       with, and bumps t's value version (plans on t turn stale until their step 3 runs, as after pem_tiled_set_values).
 *       Stream-ordered, never waits, reads nothing back and allocates nothing, not even on the first call.
 *   pem_tiled_set_values_from_scale  the same with the op t was made with; the vectors are given anew, and either may be null
 *       whatever the build had.  It allocates nothing either (the build made what it needs).
 *     Both return PEM_E_INVALID unless t was made by the matching build from exactly this A (the serial rule of
 *       pem_tiled_set_values_from_ewise: a tiling recreated at a reused address is refused), and the scale form for the wrong value
 *       type. */
typedef enum {
    /* unary: the thunk is ignored */
    PEM_APPLY_IDENTITY = 0,  /* x, bit for bit (a copy of the tiling) */
    PEM_APPLY_ABS = 1,       /* sign bit cleared; NaN stays NaN */
    PEM_APPLY_AINV = 2,      /* -x (sign bit flipped) */
    PEM_APPLY_MINV = 3,      /* 1 / x */
    PEM_APPLY_SQRT = 4,      /* sqrt(x); x < 0 gives NaN */
    PEM_APPLY_ONE = 5,       /* 1, whatever x is (NaN included); reads no values */
    /* bound to y = the thunk rounded once to the tiling's value type */
    PEM_APPLY_PLUS = 6,      /* x + y */
    PEM_APPLY_TIMES = 7,     /* x * y */
    PEM_APPLY_MIN = 8,       /* fmin(x, y) */
    PEM_APPLY_MAX = 9,       /* fmax(x, y) */
    PEM_APPLY_DIV = 10,      /* x / y */
    PEM_APPLY_RDIV = 11,     /* y / x */
    PEM_APPLY_RMINUS = 12,   /* y - x */
    PEM_APPLY_POWI = 13      /* x^k, k = thunk, an integer in 1..64: the square-and-multiply chain above */
} pem_apply_op;
pem_status pem_tiled_apply(pem_ctx *ctx, const pem_tiled *A, int op, double thunk, pem_tiled **out);
pem_status pem_tiled_set_values_from_apply(pem_ctx *ctx, pem_tiled *t, const pem_tiled *A);
pem_status pem_tiled_scale(pem_ctx *ctx, const pem_tiled *A, int op, const double *d_row, const double *d_col, pem_tiled **out);
pem_status pem_tiled_scale_f32(pem_ctx *ctx, const pem_tiled *A, int op, const float *d_row, const float *d_col, pem_tiled **out);
pem_status pem_tiled_set_values_from_scale(pem_ctx *ctx, pem_tiled *t, const pem_tiled *A, const double *d_row, const double *d_col);
pem_status pem_tiled_set_values_from_scale_f32(pem_ctx *ctx, pem_tiled *t, const pem_tiled *A, const float *d_row, const float *d_col);

/* Kronecker product (GraphBLAS GrB_kronecker): R = A (x) B under a binary op, on the device.
 *   pem_tiled_kron  a new tiling R, owning its arrays, of A.rows * B.rows rows, A.cols * B.cols columns and A's value type.  A and B
 *       must have the same value type; they may be the same handle, and either may be any tiling (converted, loaded, transpose-built,
 *       derived -- another pem_tiled_kron result included).
 *     Pattern.  Position (i * B.rows + k, j * B.cols + l) is stored exactly where A stores (i, j) and B stores (k, l), so
 *       nnz(R) = nnz(A) * nnz(B).  Explicit zeros and results that come out as 0 stay entries (the rule of sections 3f / 3g); tiles
 *       without entries are not in R (1..256 entries per tile).  An empty operand gives a valid tiling with nnz = 0.
 *     Values.  op(a, b) in the value type, rounded once, no fma and no wider intermediate; op is a pem_binop with exactly
 *       pem_tiled_ewise's both-stored arithmetic (alpha = beta = 1).  PEM_BINOP_TIMES is the Kronecker product proper; PLUS, MIN, MAX,
 *       LOR and LAND are GraphBLAS's kronecker with a binary op.  For MIN / MAX a NaN side is skipped and the sign of a zero result is
 *       not specified; a NaN that arithmetic produces has an unspecified payload.
 *     R equals the tiling pem_tiled_from_coo builds from those entries (every pem_tiled_info field but the two timings, every
 *       pem_tiled_array) and works everywhere a tiling does (A, B, mask, save / load, set_values*, flop count, split, ewise, select,
 *       extract, transpose, assign, apply, scale, mxv, spmm, sddmm, export, kron).
 *     Refusals, all before anything is launched or allocated unless noted.  PEM_E_INVALID: a null argument, an unknown op, different
 *       value types.  PEM_E_OVERFLOW: A.rows * B.rows or A.cols * B.cols exceeds INT32_MAX, or nnz(A) * nnz(B) does not fit an int32
 *       (all three computed in 64 bits on the host); and, after the tile stage has run, a tile count beyond the int32 range.
 *     A's and B's values are read as they are when the call is made (stream order); the call waits, and its allocations come from the
 *       context's arena (a captured graph re-captures once).  No entry is sorted: the only sort is over the result's candidate tiles.
 *   pem_tiled_set_values_from_kron  recomputes t's values (vals and vals_t) in place from the current values of A and B with the op t
 *       was made with, and bumps t's value version.  Stream-ordered, never waits, reads nothing back; only the first call allocates
 *       (an int32 pair per entry: where its operand values sit in A and in B).  PEM_E_INVALID unless t was made by pem_tiled_kron from
 *       exactly this A and this B in this order (the serial rule of pem_tiled_set_values_from_ewise). */
pem_status pem_tiled_kron(pem_ctx *ctx, const pem_tiled *A, const pem_tiled *B, int op, pem_tiled **out);
pem_status pem_tiled_set_values_from_kron(pem_ctx *ctx, pem_tiled *t, const pem_tiled *A, const pem_tiled *B);

/* Concat (GraphBLAS GxB_Matrix_concat): block assembly R = [[B00, B01, ..], [B10, ..], ..], on the device.
 *   pem_tiled_concat  a new tiling R, owning its arrays, from a grid of grid_rows x grid_cols tilings.  blocks is row-major with
 *       grid_rows * grid_cols entries; a null entry is an all-empty block.  row_sizes[a] and col_sizes[b] are always given: a non-null
 *       block at (a, b) is exactly row_sizes[a] x col_sizes[b].  A size of 0 is allowed (the strip contributes nothing), and so is a
 *       grid row or column of nulls only.  The same tiling may sit in several cells; a block may be any tiling (converted, loaded,
 *       derived -- another pem_tiled_concat result included); blocks without entries are ordinary blocks.
 *     R is sum(row_sizes) x sum(col_sizes) in the blocks' value type and stores (ro_a + i, co_b + j) exactly where block (a, b)
 *       stores (i, j), ro / co the exclusive prefix sums of the sizes; the value is copied bit for bit, explicit zeros stay entries.
 *       nnz(R) = the sum of the blocks' nnz (a tiling counted once per cell it sits in).  R equals the tiling pem_tiled_from_coo
 *       builds from those entries (every pem_tiled_info field but the two timings, every pem_tiled_array) and works everywhere a
 *       tiling does.  A 1 x 1 grid is a copy: R's arrays equal the block's.  The inverse is pem_tiled_extract with ranges.
 *     Refusals, all before anything is launched or allocated.  PEM_E_INVALID: a null argument, grid_rows or grid_cols < 1, a negative
 *       size, a block of the wrong shape, blocks of different value types, a block made on another context, a grid without any
 *       non-null block (there is no value type then).  PEM_E_OVERFLOW: a sum of sizes above INT32_MAX, or blocks whose entries
 *       together do not fit an int32 (both computed in 64 bits on the host).
 *     The blocks' values are read as they are when the call is made (stream order); the call waits, and its allocations come from the
 *       context's arena.  No entry is sorted: the only sort is over the result's candidate tiles.
 *   pem_tiled_set_values_from_concat  copies the blocks' current values into t (vals and vals_t) in place and bumps t's value
 *       version.  blocks is the grid again, nblocks = grid_rows * grid_cols entries with nulls where the build had nulls.
 *       Stream-ordered, never waits, reads nothing back; only the first call allocates (an int32 pair per entry: its cell and its slot
 *       in that block's values, and a pointer per cell).  PEM_E_INVALID unless t was made by pem_tiled_concat from exactly these
 *       tilings in these cells (the serial rule of pem_tiled_set_values_from_ewise): a wrong count, a swapped or foreign block and a
 *       null where the build had a block (or a block where it had a null) are refused. */
pem_status pem_tiled_concat(pem_ctx *ctx, int grid_rows, int grid_cols, const pem_tiled *const *blocks, const int64_t *row_sizes,
                            const int64_t *col_sizes, pem_tiled **out);
pem_status pem_tiled_set_values_from_concat(pem_ctx *ctx, pem_tiled *t, int nblocks, const pem_tiled *const *blocks);

/* Build from triplets that may repeat a position (GraphBLAS GrB_Matrix_build with a dup operator): the
 * duplicates of every (row, col) are folded on the device and the result is an ordinary tiling.
 *   pem_tiled_build / _device  nnz_in triplets (I, J, V) in any order -- host arrays, or device arrays read on the context's stream --
 *       become a tiling of rows x cols (transpose = 1: of the transposed matrix, as pem_tiled_from_coo) whose nnz is the number of
 *       DISTINCT positions.  pem_tiled_from_coo's argument rules hold for nnz_in: PEM_E_OVERFLOW beyond the int32 range,
 *       PEM_E_INVALID with "index out of range for a %d x %d matrix".  nnz_in = 0 and an input without duplicates are valid; the
 *       latter gives pem_tiled_from_coo_device's tiling, array for array.
 *     dup.  A pem_binop (0 .. 5), PEM_DUP_FIRST or PEM_DUP_SECOND; anything else is PEM_E_INVALID.  The duplicates of a position are
 *       folded IN INPUT ORDER, ((v0 op v1) op v2) ..., each step pem_tiled_ewise's both-stored arithmetic in the value type (MIN /
 *       MAX are fmin / fmax, LOR / LAND test != 0; a position given once keeps its value as it is under every op).  FIRST keeps the
 *       value that came first in the input, SECOND the one that came last, bit for bit.
 *     Fold order.  A position with at most PEM_BUILD_INORDER_MAX triplets is folded strictly left to right.  A longer run keeps the
 *       input order but may be regrouped: consecutive segments are folded on their own and the partial results combined in order
 *       (which rounds PLUS and TIMES differently, and nothing else).  No atomics: the same input gives the same bits every time.
 *     flags.  PEM_BUILD_KEEP_MAP keeps what pem_tiled_set_values_from_build needs (4 bytes per triplet, 4 per entry).  Without it
 *       the tiling holds exactly what pem_tiled_from_coo's tiling of the folded entries holds.
 *     The tiling works everywhere a tiling does (operand, mask, save / load, every set_values*, export, every derived route).
 *   pem_tiled_set_values_from_build  new values for the SAME triplet list (dV: nnz_in device values in the input order of the build):
 *       t's values become bit for bit what a fresh build of (I, J, dV) holds; the value version is bumped.  Stream-ordered, never
 *       waits, reads nothing back; only the first call allocates.  PEM_E_INVALID unless t was made with PEM_BUILD_KEEP_MAP from
 *       nnz_in triplets.
 *   PEM_BUILD_INORDER in the environment (a measurement knob, read when a tiling is built): an integer above PEM_BUILD_INORDER_MAX
 *       raises the run length folded strictly left to right; smaller values are ignored.  A refresh folds as its tiling's build did. */
enum { PEM_DUP_FIRST = 6, PEM_DUP_SECOND = 7 };   /* otherwise a pem_binop */
#define PEM_BUILD_KEEP_MAP 1
#define PEM_BUILD_INORDER_MAX 32
pem_status pem_tiled_build(pem_ctx *ctx, int rows, int cols, int64_t nnz_in, const int32_t *I, const int32_t *J, const double *V,
                           int transpose, int dup, int flags, pem_tiled **out);
pem_status pem_tiled_build_device(pem_ctx *ctx, int rows, int cols, int64_t nnz_in, const int32_t *dI, const int32_t *dJ,
                                  const double *dV, int transpose, int dup, int flags, pem_tiled **out);
pem_status pem_tiled_build_f32(pem_ctx *ctx, int rows, int cols, int64_t nnz_in, const int32_t *I, const int32_t *J, const float *V,
                               int transpose, int dup, int flags, pem_tiled **out);
pem_status pem_tiled_build_device_f32(pem_ctx *ctx, int rows, int cols, int64_t nnz_in, const int32_t *dI, const int32_t *dJ,
                                      const float *dV, int transpose, int dup, int flags, pem_tiled **out);
pem_status pem_tiled_set_values_from_build(pem_ctx *ctx, pem_tiled *t, const double *dV, int64_t nnz_in);
pem_status pem_tiled_set_values_from_build_f32(pem_ctx *ctx, pem_tiled *t, const float *dV, int64_t nnz_in);

/* Matrix-vector products and reductions: a tiling times a dense device vector under a semiring, and
 * the fold of every row or column, on the device.
 *   pem_tiled_mxv  y = A (+).(x) x  (transpose = 0: x has A.cols entries, y has A.rows)
 *                  y = A^T (+).(x) x  (transpose = 1: x has A.rows entries, y has A.cols)
 *     dx and dy are device arrays of the tiling's value type on the context's device; their lengths cannot be checked, so the caller
 *       provides them as above.  Coordinates are those of the matrix the tiling represents (what pem_tiled_export_csr returns): a
 *       tiling built with transpose = 1 acts as M^T.  Any tiling works (converted, loaded, from_cplan, ewise, select).
 *     Order.  Under plus-times y_i is the fma chain over row i's stored entries in ascending column, acc = fma(a_ij, x_j, acc), from 0
 *       -- or from the old y_i with accumulate = 1; for transpose = 1 y_j is the same chain over column j's entries in ascending row.
 *       The result equals, bit for bit, the plan product A*X (X: the A.cols x 1 tiling storing every x_j, zeros included) resp.
 *       X^T*A, under every semiring (section 3g's rules: each a + x and a * x rounded once in the value type, fmin / fmax skip NaN,
 *       plus_pair counts entries -- acc + 1 per entry -- reading neither x nor A's values, lor_land gives 1.0 / 0.0 with NaN != 0);
 *       min / max results do not depend on order and the sign of a zero there is not specified.  fp32 tilings compute in fp32 (fmaf).
 *       No atomics: two calls give identical bits.
 *     Empty rows (columns).  accumulate = 0: the semiring's start value (0, +inf, -inf, -inf, 0, 0).  accumulate = 1: y is left
 *       untouched there, and every other fold starts from the old y (lor_land: from y != 0).
 *   pem_tiled_reduce  y_i = the (+)-fold of row i's (dim = PEM_REDUCE_ROWS: y has A.rows entries) or column j's (PEM_REDUCE_COLS:
 *       A.cols entries) stored values, op a pem_binop: PLUS, TIMES, MIN, MAX, LOR, LAND.  A left fold in ascending index from the
 *       identity (0, 1, +inf, -inf, 0, 1), or from the old y with accumulate = 1 (LOR / LAND: from y != 0), each step rounded once;
 *       LOR / LAND give 1.0 / 0.0 (NaN != 0).  Empty rows get the identity (accumulate = 0) or stay untouched (accumulate = 1).
 *       reduce(PLUS) equals mxv(plus_times, x = 1) bit for bit; MIN / MAX equal mxv(min_plus / max_plus, x = 0) up to the sign of a
 *       zero; LOR equals mxv(lor_land, x = 1).
 *   PEM_E_INVALID: a null context or tiling; a null dx (dy) where x (y) has entries; an unknown semiring, op or dim; transpose or
 *     accumulate not 0 or 1; the fp64 form on an fp32 tiling or the reverse; x and y overlapping.  An empty tiling or a 0-length y is
 *     legal.  Stream-ordered on the context's stream; never waits and reads nothing back (a launch failure surfaces at the next
 *     synchronising call).  A's current values are read, so pem_tiled_set_values_device followed by an mxv needs no sync.  The first
 *     column-orientation call (transpose = 1, PEM_REDUCE_COLS) on a tiling builds its column schedule -- 8 bytes per tile and 1 per
 *     entry, carved from the context's arena and kept with the tiling (a captured graph re-captures once, as after the first
 *     pem_tiled_set_values); every later call allocates nothing. */
typedef enum { PEM_REDUCE_ROWS = 0, PEM_REDUCE_COLS = 1 } pem_reduce_dim;
pem_status pem_tiled_mxv(pem_ctx *ctx, const pem_tiled *A, int semiring, int transpose, const double *dx, double *dy, int accumulate);
pem_status pem_tiled_mxv_f32(pem_ctx *ctx, const pem_tiled *A, int semiring, int transpose, const float *dx, float *dy, int accumulate);
pem_status pem_tiled_reduce(pem_ctx *ctx, const pem_tiled *A, int op, int dim, double *dy, int accumulate);
pem_status pem_tiled_reduce_f32(pem_ctx *ctx, const pem_tiled *A, int op, int dim, float *dy, int accumulate);

/* Frontier products: pem_tiled_mxv with a sparse input vector and an output mask, and the breadth-first
 * search built on it.
 *   pem_tiled_mxv_frontier  orientation, lengths and coordinates as pem_tiled_mxv.  dx_present: nx bytes, x_j is present where its byte
 *       is nonzero (NULL: every x_j is present).  dy_mask: ny bytes; output i is allowed when dy_mask is NULL or (dy_mask[i] != 0) !=
 *       mask_complement.  dy_present: ny bytes, written (NULL: not wanted).  All are device arrays on the context's device (a bool or
 *       uint8 tensor works).
 *     For an allowed i, y_i is pem_tiled_mxv's fold restricted to the stored a_ij whose x_j is present: the same order (ascending j;
 *       the fma chain under plus_times), the same start value (or the old y_i with accumulate = 1), the same arithmetic, no atomics --
 *       bit for bit the plan product A*X with X the nx x 1 tiling storing exactly the present x_j (zero signs under min / max and NaN
 *       payloads excepted, as for pem_tiled_mxv).  An absent x_j is never read: whatever bytes sit there cannot reach y.  An allowed i
 *       that receives no term gets the start value (accumulate = 0) or is left untouched (accumulate = 1).  A disallowed i is never
 *       written (a mask without replace).  dy_present[i] = 1 where i is allowed and at least one term entered its fold (structural: a
 *       lor_land term that is false counts), else 0; all ny bytes are written.  plus_pair reads neither dx nor A's values: dx may be
 *       NULL there.
 *     PEM_E_INVALID, before the device is touched: the null, unknown-semiring, flag and value-type cases of pem_tiled_mxv;
 *       mask_complement not 0 or 1; dy_present's bytes overlapping dy_mask, dx_present, dx or dy; x and y overlapping.  An empty
 *       tiling and a 0-length y are legal.
 *     Stream-ordered on the context's stream; never waits and reads nothing back.  With a dx_present the call keeps 2 bytes per 16
 *       entries of x and 1 byte per 16 outputs in a grow-only scratch of the context, carved from its arena: a later call of the same
 *       or a smaller size allocates nothing.  The column orientation builds pem_tiled_mxv's column schedule on first use.  Lines no
 *       present x can reach, and lines without an allowed output, are skipped before their tile index is read; for a dense x without
 *       a mask pem_tiled_mxv is the call to use.
 *   pem_tiled_bfs  breadth-first search from `source` over the pattern of a square tiling: a stored entry (i, j), explicit zeros
 *       included, is an edge i -> j (transpose = 1: j -> i).  d_level: A.rows int32 on the device, the least number of edges from
 *       source to v, -1 where v is unreachable; *depth the largest level, *reached the number of vertices with a level.  Every level is
 *       one pem_tiled_mxv_frontier under plus_pair (frontier = dx_present, visited = the complemented mask, next frontier = dy_present)
 *       and one 4-byte read-back; no value is read.  Waits.  PEM_E_INVALID: a null argument, a tiling that is not square, source
 *       outside [0, rows), transpose not 0 or 1. */
pem_status pem_tiled_mxv_frontier(pem_ctx *ctx, const pem_tiled *A, int semiring, int transpose, const double *dx, const uint8_t *dx_present,
                                  double *dy, const uint8_t *dy_mask, int mask_complement, uint8_t *dy_present, int accumulate);
pem_status pem_tiled_mxv_frontier_f32(pem_ctx *ctx, const pem_tiled *A, int semiring, int transpose, const float *dx, const uint8_t *dx_present,
                                      float *dy, const uint8_t *dy_mask, int mask_complement, uint8_t *dy_present, int accumulate);
pem_status pem_tiled_bfs(pem_ctx *ctx, const pem_tiled *A, int64_t source, int transpose, int32_t *d_level, int32_t *depth, int64_t *reached);

/* Arg folds: where the minimum or maximum of a row's or column's fold was attained, next to -- or instead
 * of -- its value, and the breadth-first tree built on that.
 *   pem_tiled_mxv_arg  orientation, lengths, coordinates, dx_present, dy_mask / mask_complement, dy_present, stream ordering and scratch
 *       exactly as pem_tiled_mxv_frontier; dx_present = NULL and dy_mask = NULL give the dense case.  d_idx: ny int32 on the device.
 *       An entry (i, j) ENTERS the fold of an allowed output when its x is present.  Its x-index is the index into x: the column j
 *       for transpose = 0, the row i of the represented matrix for transpose = 1.  kind is a pem_arg_kind:
 *         PEM_ARG_MIN_PLUS   term a_ij + x_j, fold min;   PEM_ARG_MAX_PLUS   term a_ij + x_j, fold max;
 *         PEM_ARG_MAX_TIMES  term a_ij * x_j, fold max    (the value kinds: each term rounded once in the value type);
 *         PEM_ARG_MIN_INDEX  the smallest, PEM_ARG_MAX_INDEX the largest x-index of an entering entry (the index kinds: neither A's
 *                            values nor x are read).
 *     Value kinds, which terms win.  With accumulate = 0 every non-NaN term wins.  With accumulate = 1 a term t wins over the old y_i
 *       when the old y_i is NaN or t < y_i (the max kinds: t > y_i).  A NaN term never wins (fmin / fmax skip NaN).
 *     Value kinds, what an allowed output gets.  Where some term wins, y_i is the best winning term and idx_i the SMALLEST x-index
 *       among the terms that compare equal (==) to it: +0 and -0 tie and the lower index is reported.  Where no term wins: with
 *       accumulate = 0 y_i is the start value (+inf / -inf) and idx_i = -1; with accumulate = 1 y_i keeps the old value up to the sign
 *       of a zero and idx_i is not written.  The value written is what pem_tiled_mxv_frontier writes under the semiring of the same
 *       name for the same arguments, bit for bit (zero signs and NaN payloads excepted, as stated there).
 *     Index kinds.  dx and dy are neither read nor written; both may be NULL.  idx_i is the min (max) x-index over the entering
 *       entries; explicit zeros and NaN are entries like any other.  With accumulate = 1 the old idx_i takes part when it is >= 0.
 *       With no entering entry idx_i = -1 (accumulate = 0) or stays untouched (accumulate = 1).
 *     A disallowed output never has y, idx or anything else written.  dy_present follows pem_tiled_mxv_frontier's rule (structural: a
 *       NaN term counts).  An absent x_j is never read.  A's entries are read once per call; no atomics and no dependence on order:
 *       two calls give identical bits.
 *   pem_tiled_reduce_arg  per row (dim = PEM_REDUCE_ROWS) or column (PEM_REDUCE_COLS) the min (op = PEM_BINOP_MIN) or max
 *       (PEM_BINOP_MAX) stored value, and the smallest index inside the line where a stored value equals it; an empty line, or one
 *       whose values are all NaN, gets the identity and -1.  The values equal pem_tiled_reduce(MIN | MAX); the whole result equals
 *       pem_tiled_mxv_arg(MIN_PLUS | MAX_PLUS) with x = 0 and the same orientation (no x is allocated or read).
 *   PEM_E_INVALID, before the device is touched: the null, flag, value-type and overlap cases of pem_tiled_mxv_frontier; an unknown
 *     kind, op (only MIN and MAX have an arg) or dim; a null d_idx; under a value kind a null dy where y has entries or a null dx
 *     where x has entries; d_idx's bytes overlapping any other argument's (dx and dy do not count under an index kind).  An empty
 *     tiling and a 0-length output are legal.
 *   pem_tiled_bfs_parents  pem_tiled_bfs with the breadth-first tree: the argument checks and level semantics of pem_tiled_bfs, and
 *       d_level, *depth and *reached identical to its.  d_parent: A.rows int32 on the device, not overlapping d_level (else
 *       PEM_E_INVALID): d_parent[source] = source, -1 where v is unreachable, otherwise the smallest-numbered u of the previous level
 *       with an edge u -> v, which is deterministic.  Every level is one arg walk under PEM_ARG_MIN_INDEX (frontier = dx_present,
 *       visited = the complemented mask, the index written straight into d_parent, next frontier = dy_present) and one 4-byte
 *       read-back; no value is read.  Waits. */
typedef enum {
    PEM_ARG_MIN_PLUS = 0,
    PEM_ARG_MAX_PLUS = 1,
    PEM_ARG_MAX_TIMES = 2,
    PEM_ARG_MIN_INDEX = 3,
    PEM_ARG_MAX_INDEX = 4
} pem_arg_kind;
pem_status pem_tiled_mxv_arg(pem_ctx *ctx, const pem_tiled *A, int kind, int transpose, const double *dx, const uint8_t *dx_present, double *dy,
                             int32_t *d_idx, const uint8_t *dy_mask, int mask_complement, uint8_t *dy_present, int accumulate);
pem_status pem_tiled_mxv_arg_f32(pem_ctx *ctx, const pem_tiled *A, int kind, int transpose, const float *dx, const uint8_t *dx_present, float *dy,
                                 int32_t *d_idx, const uint8_t *dy_mask, int mask_complement, uint8_t *dy_present, int accumulate);
pem_status pem_tiled_reduce_arg(pem_ctx *ctx, const pem_tiled *A, int op, int dim, double *dy, int32_t *d_idx);
pem_status pem_tiled_reduce_arg_f32(pem_ctx *ctx, const pem_tiled *A, int op, int dim, float *dy, int32_t *d_idx);
pem_status pem_tiled_bfs_parents(pem_ctx *ctx, const pem_tiled *A, int64_t source, int transpose, int32_t *d_level, int32_t *d_parent,
                                 int32_t *depth, int64_t *reached);

/* Sparse times dense block: a tiling times k dense device vectors at once under a semiring.
 *   pem_tiled_spmm  Y = A (+).(x) X  (transpose = 0: X is A.cols x k, Y is A.rows x k)
 *                   Y = A^T (+).(x) X  (transpose = 1: X is A.rows x k, Y is A.cols x k)
 *     X and Y are row-major device arrays of the tiling's value type: element (j, c) of X is dX[j * ldx + c], and likewise for Y.
 *       They need only the value type's alignment; any ld >= max(k, 1) works.  Coordinates are those of the matrix the tiling
 *       represents, as for pem_tiled_mxv; any tiling works.
 *     Contract.  For every c, column c of Y is bit for bit what pem_tiled_mxv(A, semiring, transpose, X[:, c], y, accumulate) writes
 *       into y (with the same old y under accumulate = 1); the sign of a zero under min / max is not specified, NaN payloads are not
 *       compared.  Under plus-times each Y[i, c] is the fma chain over row i's entries in ascending column.  Empty rows: the start
 *       value (accumulate = 0) or untouched (accumulate = 1).  No atomics: two calls give identical bits.  Columns [k, ldy) of Y are
 *       never written.
 *   PEM_E_INVALID: a null context or tiling; an unknown semiring; transpose or accumulate not 0 or 1; k < 0; ldx or ldy below
 *     max(k, 1); a null dX (dY) where X (Y) has entries; the fp64 form on an fp32 tiling or the reverse; X's and Y's byte spans
 *     overlapping (a span runs from p to p + ((n - 1) * ld + k) * value_bytes); n * ld overflowing int64.  k = 0, a 0-row Y and an
 *     empty tiling are legal.  Stream-ordered on the context's stream; never waits and reads nothing back.  A's current values are
 *     read.  Allocates nothing, except that the first column-orientation call on a tiling builds the column schedule pem_tiled_mxv
 *     keeps with it (see above). */
pem_status pem_tiled_spmm(pem_ctx *ctx, const pem_tiled *A, int semiring, int transpose, int64_t k, const double *dX, int64_t ldx,
                          double *dY, int64_t ldy, int accumulate);
pem_status pem_tiled_spmm_f32(pem_ctx *ctx, const pem_tiled *A, int semiring, int transpose, int64_t k, const float *dX, int64_t ldx,
                              float *dY, int64_t ldy, int accumulate);

/* Sampled dense-dense product, SDDMM: R = pattern(S) o (X . Y^T) under a semiring, on the device.
 *   X is rows x k and Y is cols x k, rows and cols those of the matrix the tiling represents (what pem_tiled_export_csr returns: a
 *     tiling built with transpose = 1 is its own matrix).  Both are row-major device arrays of the entry point's value type with
 *     row strides ldx, ldy >= max(k, 1): element (i, c) of X is dX[i * ldx + c].  They need only the value type's alignment, are
 *     read-only, and may alias or be the same pointer (H . H^T).
 *   For every stored position (i, j):  R(i, j) = (+)_{c = 0 .. k-1} X[i, c] (x) Y[j, c], with section 3g's arithmetic: plus_times
 *     is the chain acc = fma(X[i, c], Y[j, c], acc) in ascending c from 0 (fmaf for fp32); min_plus / max_plus / max_times round
 *     each + / * once and fold with fmin / fmax from +-inf (NaN terms skipped, the sign of a zero result not specified); plus_pair
 *     stores k (acc + 1 per column) without reading X or Y; lor_land stores 1.0 if some c has both operands != 0 (NaN counts as
 *     != 0), else 0.0.  k = 0 stores the semiring's start value (0, +inf, -inf, -inf, 0, 0) everywhere.  The pattern is never
 *     touched: zeros that come out stay entries.  NaN payloads are not specified.  The stored values of S / the old values of t are
 *     never read (with accumulate = 0): S o (X . Y^T) scaled by S's values is pem_tiled_ewise(S, R, PEM_EWISE_INTERSECT,
 *     PEM_BINOP_TIMES).
 *   pem_tiled_sddmm  a new tiling R with S's pattern, holding the sampled product in the entry point's value type (S may hold either
 *       value type, as a mask may).  R owns its arrays and works everywhere a tiling does (A, B, mask, save / load, set_values*,
 *       ewise, select, mxv, spmm, export, and a later pem_tiled_set_values_sddmm on R itself for the next X, Y).  It equals, every
 *       pem_tiled_array and every pem_tiled_info field but the two timings, the tiling pem_tiled_from_csr builds from S's exported
 *       pattern with these values.  The call waits, like the other builders; its allocations come from the context's arena.  An S
 *       with nnz = 0 gives a valid empty tiling.
 *   pem_tiled_set_values_sddmm  in place: t's values (vals and vals_t) become the sampled product at t's own pattern; t must hold the
 *       entry point's value type (the rule of pem_tiled_set_values*).  accumulate = 1: every fold starts from the entry's old value
 *       (lor_land: from old != 0), so one call with k = k1 + k2 equals a call on columns [0, k1) followed by an accumulate call on
 *       columns [k1, k1 + k2), bit for bit (zero signs under min / max excepted).  Bumps t's value version (plans built on t turn
 *       stale under the rule of pem_tiled_set_values).  Stream-ordered on the context's stream, never waits, reads nothing back;
 *       allocates only on the tiling's first refresh (the vals_t map of pem_tiled_set_values, an arena allocation: a captured graph
 *       re-captures once).  No atomics, every value is written once: two calls give identical bits.
 *   PEM_E_INVALID: a null context, tiling or out; an unknown semiring; accumulate not 0 or 1; k < 0; ldx or ldy below max(k, 1); a
 *     null dX (dY) where X (Y) has elements and the semiring reads them (every semiring but plus_pair); n * ld overflowing int64;
 *     the in-place fp64 form on an fp32 tiling or the reverse.  All of these are checked before the device is touched. */
pem_status pem_tiled_set_values_sddmm(pem_ctx *ctx, pem_tiled *t, int semiring, int64_t k, const double *dX, int64_t ldx, const double *dY,
                                      int64_t ldy, int accumulate);
pem_status pem_tiled_set_values_sddmm_f32(pem_ctx *ctx, pem_tiled *t, int semiring, int64_t k, const float *dX, int64_t ldx, const float *dY,
                                          int64_t ldy, int accumulate);
pem_status pem_tiled_sddmm(pem_ctx *ctx, const pem_tiled *S, int semiring, int64_t k, const double *dX, int64_t ldx, const double *dY,
                           int64_t ldy, pem_tiled **out);
pem_status pem_tiled_sddmm_f32(pem_ctx *ctx, const pem_tiled *S, int semiring, int64_t k, const float *dX, int64_t ldx, const float *dY,
                               int64_t ldy, pem_tiled **out);

/* Sampled sparse product: R = pattern(S) o (A * B) under a semiring, by dot products, on the device.
 * Where SDDMM samples a dense product, this samples a sparse one; where the masked plan C<S> = A * B lists every tile-level product
 * of A and B and then filters, this reads only the tile lists S's tiles touch: the cost follows S, not flop(A * B).
 *   transpose_b = 0: A is m x n, B is n x p, S (or t) is m x p.  transpose_b = 1: B is p x n and the product is A * B^T (no
 *     transposed tiling is needed).  Coordinates are those of the matrix each tiling represents (what pem_tiled_export_csr returns:
 *     a tiling built with transpose = 1 is its own matrix).
 *   For every stored position (i, j) of the pattern, R(i, j) is the fold over every k, in ascending k, where A(i, k) is stored and
 *     B(k, j) is stored (transpose_b = 1: B(j, k)), with step 3's arithmetic (section 3g): plus_times is the chain acc = fma(a, b,
 *     acc) from 0 (fmaf for fp32); min_plus / max_plus / max_times round each + / * once and fold with fmin / fmax from +-inf;
 *     plus_pair counts the k's and reads no value; lor_land gives 1.0 / 0.0 with NaN counting as != 0.  A position that no k reaches
 *     gets the semiring's start value (0, +inf, -inf, -inf, 0, 0), as SDDMM does at k = 0.  The pattern is never touched: zeros and
 *     start values stay entries.  The stored values of S / the old values of t are never read (with accumulate = 0).  No atomics,
 *     every value is written once: two calls give identical bits.
 *   Consequences.  (1) Where the masked plan C<S> = A * B (transpose_b = 1: with pem_tiled_transpose(B) as its B) stores (i, j),
 *     R(i, j) equals its value bit for bit; elsewhere in S's pattern R holds the start value.  (2) Under plus_pair,
 *     pem_tiled_select(R, PEM_SELECT_VALUE_NE, 0) has exactly the masked plan's pattern.  (3) Split A's columns, and B's rows to
 *     match, at any n1: a call on (A1, B1) followed by an accumulate call on (A2, B2) equals one call on (A, B), bit for bit (zero
 *     signs under min / max excepted).
 *   pem_tiled_sampled_mxm  a new tiling R with S's pattern and A's value type (S may hold either value type, as a mask may).  R owns
 *       its arrays and works everywhere a tiling does.  It equals, every pem_tiled_array and every pem_tiled_info field but the two
 *       timings, the tiling pem_tiled_from_csr builds from S's exported pattern with these values.  The call waits, like the other
 *       builders; its allocations come from the context's arena.  An S with nnz = 0 gives a valid empty tiling.  S, A and B may be
 *       the same handle in any combination (L o (L * L^T) is pem_tiled_sampled_mxm(ctx, L, L, L, 1, ..)).
 *   pem_tiled_set_values_sampled_mxm  in place, on t's own pattern: t's values (vals and vals_t, written by the same kernel) become
 *       the sampled product; t must hold A's value type.  accumulate = 1: every fold starts from the entry's old value (lor_land:
 *       from old != 0; plus_pair: the count of a tile pair enters in one addition, which equals one addition per k while the
 *       value is an integer below 2^24 (fp32) / 2^53).  Bumps t's value version (plans built on t turn stale under the rule of
 *       pem_tiled_set_values).  Stream-ordered, never waits, reads nothing back; A's and B's current values are read.  Allocates
 *       only on the tiling's first refresh (the vals_t map of pem_tiled_set_values); the tile intersections are searched again by
 *       every call, not kept.
 *   One untyped pair serves fp64 and fp32 (as pem_tiled_select): no host or device value array crosses the ABI.
 *   PEM_E_INVALID, all checked before the device is touched (*out stays NULL): a null context, tiling or out; an unknown semiring;
 *     transpose_b or accumulate not 0 or 1; A and B of different value types; t of another value type than A; inner dimensions that
 *     differ; a pattern shape that is not m x p; t == A or t == B (the refresh would read what it writes).
 *   PEM_SAMPLED_LPT in the environment (a measurement knob, read at every call): 16 packs four pattern tiles into a wave (16 lanes
 *     each), 64 gives every pattern tile a wave; other values are ignored.  The results do not depend on it. */
pem_status pem_tiled_sampled_mxm(pem_ctx *ctx, const pem_tiled *S, const pem_tiled *A, const pem_tiled *B, int transpose_b, int semiring,
                                 pem_tiled **out);
pem_status pem_tiled_set_values_sampled_mxm(pem_ctx *ctx, pem_tiled *t, const pem_tiled *A, const pem_tiled *B, int transpose_b,
                                            int semiring, int accumulate);

/* Triangular solve: x = T^-1 b on the device, T the lower or upper triangle of a square tiling.
 *   pem_tiled_trsv  A must be square (n = A.rows); coordinates are those of the matrix the tiling represents, as for pem_tiled_mxv.
 *       T is the chosen triangle of A AS STORED: entries on the other side of the diagonal are ignored (the BLAS uplo convention), so
 *       a full A serves Gauss-Seidel directly.  With unit_diag = 1 the stored diagonal entries are ignored as well and the diagonal
 *       counts as 1.  db and dx are device arrays of n values of the tiling's value type; dx == db (the in-place solve) is legal.
 *     Order (bit-exact; P = i / 16, the tile size of the format -- pem_tiled_get_array):
 *       lower, rows ascending.  acc = b_i; for the stored a_ij with j < i in ascending j: acc = fma(-a_ij, x_j, acc); then
 *         x_i = acc / a_ii, one IEEE division, or x_i = acc under unit_diag.
 *       upper, rows descending.  acc = b_i; first the stored a_ij with j >= 16 (P + 1) in ascending j, then those with
 *         i < j < 16 (P + 1) in descending j, the same fma; then the division.
 *       fp32 tilings compute in fp32 (fmaf, fp32 division).  No atomics: two calls give identical bits.  A zero, infinite or NaN
 *       diagonal value is no error: the division gives what IEEE gives.
 *     PEM_E_INVALID: a null context or tiling; rows != cols; uplo or unit_diag not 0 or 1; the fp64 form on an fp32 tiling or the
 *       reverse; a null db or dx where n > 0; db and dx overlapping other than exactly; with unit_diag = 0 a row without a stored
 *       diagonal entry (the message names the first such row, 1-based).  n = 0, and an empty tiling under unit_diag, are legal.
 *     Schedule.  The first call per (tiling, uplo) builds the dependency schedule and keeps it with the tiling: tile row P (16 rows)
 *       waits for tile row Q wherever tile (P, Q) is stored on the chosen side; level(P) = 1 + the largest level it waits for.  That
 *       call reads the tile CSR back (two int arrays, no entry-level data), counts the rows without a stored diagonal on the device,
 *       carves one buffer (24 bytes per tile row) from the context's arena and waits.  Every later call allocates nothing, is
 *       ordered on the context's stream, never waits and reads nothing back; pem_tiled_set_values* keeps the schedule.  A level wider
 *       than merge_width tile rows is one kernel launch; a maximal run of consecutive levels each at most merge_width wide is one
 *       launch of one workgroup.  No kernel waits on what another workgroup writes in the same launch.
 *   pem_tiled_trsv_info  the schedule of a triangle (built if need be; same refusals for ctx, A, uplo; a null out): levels, the
 *       launches of one solve, the widest level in tile rows, merge_width, the rows without a stored diagonal entry and the first of
 *       them (1-based; 0 if none).  All 0 but merge_width for n = 0. */
enum { PEM_TRSV_LOWER = 0, PEM_TRSV_UPPER = 1 };
pem_status pem_tiled_trsv(pem_ctx *ctx, const pem_tiled *A, int uplo, int unit_diag, const double *db, double *dx);
pem_status pem_tiled_trsv_f32(pem_ctx *ctx, const pem_tiled *A, int uplo, int unit_diag, const float *db, float *dx);
typedef struct {
    int64_t levels, launches, max_width, merge_width, missing_diag, first_missing_row;
} pem_trsv_info;
pem_status pem_tiled_trsv_info(pem_ctx *ctx, const pem_tiled *A, int uplo, pem_trsv_info *out);

/* ILU(0): the incomplete LU of a square tiling on its own pattern, on the device.
 *   pem_tiled_ilu0  A is square with stored pattern S (coordinates of the matrix the tiling represents).  *out is a new tiling F
 *       with exactly A's pattern and value type that stores L's strict lower triangle and U with its diagonal in one tiling; L has
 *       a unit diagonal, which is not stored.  Nothing is ever dropped from the pattern and nothing is added to it.
 *     Order (bit-exact).  With m = min(i, j), for every stored (i, j):
 *         acc = a_ij;  for k ascending over { k < m : (i, k) in S and (k, j) in S }: acc = fma(-f_ik, f_kj, acc);
 *         f_ij = acc / f_jj where j < i (one IEEE division, correctly rounded, in the value type), else f_ij = acc.
 *       fp32 tilings compute in fp32 (fmaf, fp32 division), fp64 tilings in fp64.  No atomics: the same bits on every call and on
 *       every launch route.  A position that is not stored is never multiplied -- it is not a zero: an infinite f_ik next to an
 *       unstored (k, j) leaves f_ij untouched.  A zero, infinite or NaN pivot is no error: the division gives what IEEE gives.
 *     F is an ordinary tiling (export, save / load, mxv, transpose, operand of a plan).  The preconditioner solve z = U^-1 L^-1 r is
 *       pem_tiled_trsv(ctx, F, PEM_TRSV_LOWER, 1, r, t) then pem_tiled_trsv(ctx, F, PEM_TRSV_UPPER, 0, t, z): no select needed.
 *     Schedule: the lower triangle's of pem_tiled_trsv (tile row P waits for Q wherever tile (P, Q), Q < P, is stored), built for F
 *       by this call and kept; a level wider than merge_width tile rows is one launch, a maximal run of narrower levels one launch of
 *       one workgroup.  Waits; allocates from the context's arena.
 *     PEM_E_INVALID (*out stays NULL): a null argument; rows != cols; a row without a stored diagonal entry (the message names the
 *       first such row, 1-based).
 *   pem_tiled_set_values_from_ilu0  recomputes F from A's current values (after pem_tiled_set_values* on A) and bumps F's value
 *       version.  Stream-ordered: never waits, reads nothing back, allocates nothing; F's trsv schedules stay.  F must have been
 *       made by pem_tiled_ilu0 from exactly this A, else PEM_E_INVALID (the rule of the other pem_tiled_set_values_from_*).
 *   pem_tiled_ilu0_info  of a square tiling F: the levels, launches, widest level and merge width of the factorisation's launch
 *       plan; zero_pivots, the rows whose f_ii is +-0, not finite or not stored, and the first of them (1-based; 0 if none).  One
 *       small kernel over the diagonal and two scalars read back: the only one of the three that has to synchronise on a factor.
 *   Not covered: IC(0), fill levels above 0, pivoting, diagonal shifts, a pem_mgpu_* path. */
pem_status pem_tiled_ilu0(pem_ctx *ctx, const pem_tiled *A, pem_tiled **out);
pem_status pem_tiled_set_values_from_ilu0(pem_ctx *ctx, pem_tiled *F, const pem_tiled *A);
typedef struct {
    int64_t levels, launches, max_width, merge_width, zero_pivots, first_zero_pivot_row;
} pem_ilu0_info;
pem_status pem_tiled_ilu0_info(pem_ctx *ctx, const pem_tiled *F, pem_ilu0_info *out);

/* Graph colouring: the greedy colouring of a square tiling's pattern, and the permutation that sorts the
 * vertices by colour -- what reorders a matrix so that pem_tiled_trsv and pem_tiled_ilu0 have few levels -- on the device.
 *   pem_tiled_colour  A is square (n = A.rows) and of either value type; values are never read.  The vertices are 0 .. n - 1; every
 *       stored entry (i, j) with i != j, explicit zeros and NaN included, is an UNDIRECTED edge {i, j}; diagonal entries are ignored.
 *       symmetric = 0: both directions are seen whatever is stored, so an edge stored one way counts.  symmetric = 1: the caller
 *       promises a symmetric pattern and only the row orientation is walked; on a symmetric pattern the result is identical to
 *       symmetric = 0.  Where the promise is false the call still ends and writes a colour in [0, n) everywhere; the colours are
 *       otherwise unspecified.
 *     Priorities.  d_priority == NULL: the priority of v is fmix32((uint32_t)v + seed * 0x9E3779B9u) in 32-bit wrap-around
 *       arithmetic, fmix32(h): h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16 -- a bijection, so no two
 *       vertices tie.  It is computed in registers: no priority array exists.  d_priority != NULL: n uint32 on the device, larger
 *       first; seed is ignored.  Ties go to the LOWER index, so all-equal priorities give the natural-order greedy colouring.
 *     The result is fully determined: d_colour[v] (n int32 on the device) is the smallest colour >= 0 that no neighbour of higher
 *       priority holds -- the sequential greedy colouring in descending (priority, -index) order.  *ncolours = the largest colour
 *       + 1; *rounds = the number of vertices on the longest chain of neighbours with strictly falling priority (an isolated vertex
 *       is coloured in round 1); both 0 for n = 0.  Two calls give identical arrays.
 *     Rounds (Jones-Plassmann).  In a round every uncoloured vertex that no uncoloured neighbour beats takes its colour.  A round
 *       reads one colour buffer and writes another: no kernel reads a colour the same launch writes, nothing waits on another
 *       workgroup.  One 4-byte read-back per round; waits.  The second buffer is a grow-only allocation of the context (4 n bytes,
 *       carved from its arena): a later call of the same or a smaller size allocates nothing.  symmetric = 0 builds
 *       pem_tiled_mxv's column schedule on first use.
 *     PEM_E_INVALID, before the device is touched: a null ctx, A, d_colour, ncolours or rounds; a tiling that is not square;
 *       symmetric not 0 or 1; d_priority overlapping d_colour.  An empty tiling and n = 0 are legal.
 *   pem_colour_order  the stable counting sort by colour.  d_colour: n int32 in [0, ncolours).  d_perm: n int32, the vertices
 *       colour by colour, ascending inside a colour (numpy's argsort(colour, kind="stable")); d_offsets: ncolours + 1 int32, colour c
 *       is d_perm[d_offsets[c] .. d_offsets[c + 1]).  d_perm goes straight into pem_tiled_extract_device as both lists.  One wait; the
 *       sort's buffers (24 n bytes) share the context's grow-only allocation with pem_tiled_colour.  Any int32 key in [0, ncolours)
 *       sorts: the component ids of pem_tiled_components with ncolours = its *ncomponents give the component order (the radix
 *       sort takes the bits of ncolours, whatever its size).
 *     PEM_E_INVALID, before the device is touched: a null argument; n < 0 or n > INT32_MAX; ncolours < 0; ncolours = 0 with n > 0;
 *       overlapping arrays.  A colour outside [0, ncolours) is found on the device and gives PEM_E_INVALID after the call's wait; the
 *       outputs are then unspecified, but nothing is written outside them. */
pem_status pem_tiled_colour(pem_ctx *ctx, const pem_tiled *A, int symmetric, uint32_t seed, const uint32_t *d_priority, int32_t *d_colour,
                            int32_t *ncolours, int32_t *rounds);
pem_status pem_colour_order(pem_ctx *ctx, int64_t n, const int32_t *d_colour, int32_t ncolours, int32_t *d_perm, int32_t *d_offsets);

/* Connected components: the components of a square tiling's pattern -- what splits a matrix that falls
 * apart into independent blocks before pem_tiled_ilu0 and pem_tiled_trsv -- on the device.
 *   pem_tiled_components  A is square (n = A.rows) and of either value type; values are never read.  The vertices are 0 .. n - 1;
 *       every stored entry (i, j), explicit zeros and NaN included, is the UNDIRECTED edge {i, j}; a diagonal entry changes nothing.
 *       symmetric = 0: both orientations are walked, as in pem_tiled_colour, so an edge stored one way counts: the weakly connected
 *       components.  symmetric = 1: the caller promises a symmetric pattern and only the row orientation is walked; on a symmetric
 *       pattern labels, ids, count and rounds are identical to symmetric = 0.  Where the promise is false the call still ends,
 *       returns PEM_OK and writes 0 <= d_label[v] <= v everywhere; the values are otherwise unspecified.
 *     The result is fully determined: d_label[v] (n int32 on the device) is the smallest vertex number in v's component.  d_id[v]
 *       (n int32 on the device; d_id may be NULL) is the number of components whose smallest vertex is below d_label[v]: the dense
 *       ids 0 .. *ncomponents - 1 in order of smallest vertex.  *ncomponents = the number of v with d_label[v] == v.  *rounds = the
 *       number of rounds below that ran, the last one (which changes nothing) included: 1 for a graph without off-diagonal entries.
 *       Both counts are 0 for n = 0.  Two calls give identical arrays and counts.
 *     A round.  The state is a parent array f, started at f[v] = v.  gp[v] = f[f[v]]; m[v] = the minimum of gp[u] over the
 *       neighbours u of v (none for a vertex without entries); f'[x] = min(gp[x], m[x], min{m[v] : f[v] == x}) -- FastSV's
 *       shortcutting, aggressive hooking and hooking onto the parent, taken on one snapshot.  The call ends after the first round
 *       with f' == f.  f' is a minimum over a fixed set, so it does not depend on any order: the rounds are determined although
 *       the hooks are integer atomicMins.  No kernel plain-reads an array the same launch writes or hits with atomics, nothing
 *       waits on another workgroup.  With both orientations walked f after t rounds is at most the smallest vertex within distance
 *       t, so at most n rounds run; the loop never runs more: with symmetric = 0 a round n that still changed something is
 *       PEM_E_HIP ("internal"), with symmetric = 1 the loop stops there with PEM_OK (the promise was false).
 *     One 4-byte read-back per round; waits.  The scratch -- two buffers of n + 1 int32 (with d_label the three a round reads and
 *       writes; the first then holds the root flags the ids' scan takes, in place) and the round words -- is the context's grow-only
 *       allocation that pem_tiled_colour and pem_colour_order use (carved from its arena): a later call of the same or a smaller
 *       size allocates nothing.  symmetric = 0 builds pem_tiled_mxv's column schedule on first use.
 *     PEM_E_INVALID, before the device is touched: a null ctx, A, d_label, ncomponents or rounds; a tiling that is not square;
 *       symmetric not 0 or 1; d_id overlapping d_label.  An empty tiling and n = 0 are legal.
 *   The component order is pem_colour_order(ctx, n, d_id, ncomponents, d_perm, d_offsets): the ids are valid keys (see above). */
pem_status pem_tiled_components(pem_ctx *ctx, const pem_tiled *A, int symmetric, int32_t *d_label, int32_t *d_id /* may be NULL */,
                                int64_t *ncomponents, int32_t *rounds);

/* Independent sets and aggregation: a maximal independent set at distance 1 or 2 of a square tiling's
 * pattern and the MIS(2) aggregation (Bell, Dalton, Olson) on top of it -- the first step of an algebraic-multigrid level, what
 * makes the P of P^T (A P) -- on the device.
 *   The graph, the priorities and "beats" are pem_tiled_colour's: A is square (n = A.rows) and of either value type, values are
 *       never read; every stored off-diagonal (i, j), explicit zeros and NaN included, is the UNDIRECTED edge {i, j}.  symmetric = 0
 *       walks the row line and the column line (pem_tiled_mxv's column schedule, built on first use); symmetric = 1 is the caller's
 *       promise of a symmetric pattern and only rows are walked.  The priority of v is fmix32(v + seed * 0x9E3779B9) computed in
 *       registers when d_priority is NULL, else d_priority[v] (n uint32 on the device).  u BEATS v when prio[u] > prio[v], or the two
 *       are equal and u < v.  Distance is path length in this undirected graph.
 *   pem_tiled_mis  d_in_set (n bytes on the device, 0 / 1) is the set the sequential greedy pass builds: the vertices are taken in
 *       "beats" order and v enters iff no vertex already in the set lies within `distance` (1 or 2) of v.  It is independent and
 *       maximal at that distance; a vertex without off-diagonal entries is always in it.  *count is its size.
 *     The device runs rounds on a three-valued state -- undecided, in, out; all start undecided -- every round taken from one
 *       snapshot: an undecided v with an in vertex within `distance` turns out; otherwise an undecided v that no undecided vertex
 *       within `distance` beats turns in; everything else stays.  Out vertices still relay: distance 2 through an out (or in) middle
 *       vertex counts.  The call ends after the first round that leaves no undecided vertex; *rounds counts the rounds that ran: 1
 *       for a graph without edges, 0 for n = 0.  The rounds reproduce the greedy set exactly and every decision is a maximum over a
 *       fixed set, so set, count and rounds are fully determined.  Every round decides at least the best undecided vertex, so at
 *       most n rounds run: with symmetric = 0 a round n that leaves an undecided vertex is PEM_E_HIP ("internal"); with
 *       symmetric = 1 (a false promise) the loop stops there with PEM_OK, and every byte of d_in_set is 0 or 1.
 *   pem_tiled_aggregate  The roots are pem_tiled_mis at distance 2 with the same arguments; *rounds is its rounds.  The roots are
 *       numbered densely in ascending vertex order; *naggregates is their number; d_root[c] (n int32 on the device, may be NULL) is
 *       the root of aggregate c, entries from *naggregates up to n are -1.  Pass 1: a non-root v with a root neighbour joins that
 *       root's aggregate (on an undirected graph there is at most one; where a false promise shows several, the one that beats the
 *       others).  Pass 2: a v still without an aggregate takes, of its neighbours that pass 1 placed, the u that beats the others and
 *       joins d_aggregate[u]; what pass 2 itself places is not seen.  On an undirected graph every vertex is placed, every
 *       aggregate holds exactly one root, is connected and has radius <= 2 around its root, and a vertex without edges is an
 *       aggregate of one.  Under a false symmetric = 1 promise a vertex may keep -1; everything written lies in [-1, *naggregates).
 *   Both: PEM_E_INVALID, before the device is touched: a null ctx, A, output array (d_in_set, d_aggregate) or count pointer; a
 *       tiling that is not square; distance not 1 or 2; symmetric not 0 or 1; d_priority overlapping an output; d_aggregate
 *       overlapping d_root.  An empty tiling and n = 0 are legal.  One 4-byte read-back per round; waits.  No kernel plain-reads, at
 *       another vertex, an array the same launch writes; nothing waits on another workgroup.  The scratch (state bytes, the 8-byte
 *       first-hop maxima, the scan's flags, a second aggregate buffer, the round words) is the context's grow-only allocation
 *       pem_tiled_colour uses: a later call of the same or a smaller size allocates nothing. */
pem_status pem_tiled_mis(pem_ctx *ctx, const pem_tiled *A, int distance /* 1 or 2 */, int symmetric, uint32_t seed,
                         const uint32_t *d_priority /* may be NULL */, uint8_t *d_in_set /* n bytes, 0 / 1 */, int64_t *count, int32_t *rounds);
pem_status pem_tiled_aggregate(pem_ctx *ctx, const pem_tiled *A, int symmetric, uint32_t seed, const uint32_t *d_priority /* may be NULL */,
                               int32_t *d_aggregate /* n */, int32_t *d_root /* n, may be NULL */, int64_t *naggregates, int32_t *rounds);

/* Krylov solvers: A x = b by preconditioned conjugate gradients (CG, for symmetric positive definite A)
 * or right-preconditioned BiCGStab, on the device.  The whole loop runs on the context's stream; the host reads one small state block
 * back every check_every iterations.
 *   pem_krylov_create  A is square (n = A.rows).  precond: PEM_PRECOND_NONE (z = r), PEM_PRECOND_DIAG (z_i = minv_i * r_i, minv an
 *       argument of every solve) or PEM_PRECOND_LU: F is a square tiling of A's size and value type with a stored diagonal -- usually
 *       pem_tiled_ilu0(A) -- applied as pem_tiled_trsv(F, LOWER, unit_diag = 1, r, w) then pem_tiled_trsv(F, UPPER, 0, w, z).  The
 *       call builds the trsv schedules of both triangles of F, so no solve builds one, and carves every work vector (CG: r, p, q,
 *       with LU also z and the trsv work vector w; BiCGStab: r, rhat, p, v, s, t, with DIAG or LU also y and z, with LU also w), seven
 *       partial slots of 1024 doubles and two 128-byte state blocks from the context's arena in one block.  May wait.
 *     The object holds handles, not copies: every solve reads the current values of A and F, so pem_tiled_set_values* on A or
 *       pem_tiled_set_values_from_ilu0 on F between solves needs nothing rebuilt.  A and F must outlive it (the rule of plans).
 *     PEM_E_INVALID, before the device is touched (*out stays NULL): a null ctx, A, opts or out; rows != cols; an unknown method or
 *       preconditioner; F missing under LU, or F given under another preconditioner; F of another size or value type; max_iters
 *       < 0; check_every < 1; rtol or atol negative or NaN.  A row of F without a stored diagonal entry gives pem_tiled_trsv's
 *       message (PEM_E_INVALID, after the schedule was built).
 *   pem_krylov_solve  db, dx (in: the guess x0; out: x), d_minv (DIAG only; ignored otherwise) hold n values of the tiling's value
 *       type on the device; d_history, if not NULL, max_iters + 1 doubles on the device.  Allocates nothing; ordered on the context's
 *       stream; waits only for its state read-backs.  PEM_E_INVALID: a null ctx, solver or res; another context than create's; the fp64
 *       form on an fp32 tiling or the reverse; a null db or dx where n > 0; d_minv null under DIAG; any two of db, dx, d_minv,
 *       d_history overlapping.  n = 0 is legal: CONVERGED, 0 iterations, nothing launched.
 *   pem_krylov_destroy  frees the object (its block goes back to the arena).
 *
 *   THE ORDER IS THE CONTRACT: x and the written part of d_history are fully determined, bit for bit.
 *     Arithmetic.  VT = the tiling's value type.  The vector updates use no fma: every product and every sum below is rounded once
 *       in VT, in the order the parentheses give.  All scalars (dots, alpha, beta, omega, rho, the threshold) are fp64, computed with
 *       one IEEE operation per operator written; a scalar is rounded once to VT before it multiplies a vector.  A x is
 *       pem_tiled_mxv's fma chain, the LU preconditioner pem_tiled_trsv's.
 *     dot(u, v).  fp64 for both value types (an fp32 product is exact in fp64).  The partition depends on n alone: chunks of 4096
 *       elements; G = min(ceil(n / 4096), 1024) workgroups of 256 threads; workgroup g takes the chunks g, g + G, ...; thread t of it
 *       the elements chunk * 4096 + t + 256 j, j = 0 .. 15 (one element per load).  A thread keeps ONE chain acc = acc + u_i * v_i
 *       from +0.0 in ascending i.  Lane l of a wave (t = 64 w + l) then does acc = acc + (acc of lane l xor m) for m = 32, 16, 8, 4,
 *       2, 1; the four waves combine as (w0 + w1) + (w2 + w3): partial[g].  The total: thread t chains partial[t], partial[t + 256],
 *       partial[t + 512], partial[t + 768] (those below G) from +0.0 in that order, then the same wave and workgroup tree.
 *     Launch rules.  No floating-point atomics; no kernel reads what the same launch writes; nothing waits on another workgroup.  A
 *       dot's partials are written by one kernel and totalled in the prologue of the next solver kernel, by every workgroup in the
 *       same order; workgroup 0 alone writes the scalars and the state, into the state block the launch does not read.
 *     Start (both methods).  q = A x; r_i = b_i - q_i; bb = dot(b, b); rr = dot(r, r); t1 = (rtol * rtol) * bb; t2 = atol * atol;
 *       threshold = t1 > t2 ? t1 : t2; history[0] = rr.  CHECK(k): rr not finite -> NONFINITE; else rr <= threshold -> CONVERGED; else
 *       k == max_iters -> MAX_ITERS; iters = k in all three.  The start ends with CHECK(0).
 *     CG.  z = M^-1 r; rz = dot(r, z); p = z.  For k = 1, 2, ...:
 *         q = A p; pq = dot(p, q); not (pq > 0) or pq not finite -> BREAKDOWN, iters = k - 1, x as after k - 1;
 *         alpha = rz / pq; x_i = x_i + alpha * p_i; r_i = r_i - alpha * q_i; z = M^-1 r; rr = dot(r, r); rz' = dot(r, z);
 *         history[k] = rr; CHECK(k); beta = rz' / rz; p_i = z_i + beta * p_i; rz = rz'.
 *     BiCGStab, right-preconditioned.  rhat = r; rho' = rr; rho' == 0 or not finite -> BREAKDOWN (iters 0); p = r.  For k = 1, 2, ...:
 *         y = M^-1 p; v = A y; rv = dot(rhat, v); rv == 0 or not finite -> BREAKDOWN (iters k - 1, x as after k - 1);
 *         alpha = rho' / rv; s_i = r_i - alpha * v_i; ss = dot(s, s);
 *         ss <= threshold -> x_i = x_i + alpha * y_i; history[k] = ss; rr = ss; CONVERGED, iters = k;
 *         z = M^-1 s; t = A z; ts = dot(t, s); tt = dot(t, t); not (tt > 0) or tt not finite -> BREAKDOWN (iters k - 1, x as after k - 1);
 *         omega = ts / tt; x_i = (x_i + alpha * y_i) + omega * z_i; r_i = s_i - omega * t_i; rr = dot(r, r); rho = rho';
 *         rho' = dot(rhat, r); history[k] = rr; CHECK(k); omega == 0 -> BREAKDOWN (iters k); rho' == 0 or not finite -> BREAKDOWN
 *         (iters k); beta = (rho' / rho) * (alpha / omega); p_i = r_i + beta * (p_i - omega * v_i).
 *     The preconditioner.  NONE: z = r, no copy.  DIAG: z_i = minv_i * r_i, one product in VT.  LU: the two solves above.
 *     Stopping.  The decision is taken on the device.  Once a status is set every later solver kernel of the call leaves x, r, p,
 *       the scalars and d_history untouched (the mxv and trsv launches in between write scratch vectors only).  The host enqueues
 *       min(check_every, what is left of max_iters) iterations, reads the 128-byte state block back (one read-back) and stops when
 *       the status is set: x, iters, status and the written part of d_history are identical for every check_every; entries of
 *       d_history after iters are not written, entries 0 .. iters all are.  With E = min(max_iters, check_every * readbacks) the iterations enqueued and T the launches of the
 *       two trsv calls (pem_tiled_trsv_info): res->readbacks = max(1, ceil(K / check_every)), K the iteration during which the status
 *       was set (0: at the start); res->launches = S + E * I, the start S = 3 (CG with LU: 4 + T) and an iteration I = 4 for CG
 *       (LU: 5 + T) and 7 for BiCGStab (LU: 7 + 2 T), the mxv launches included.
 *     The solver's own kernels per iteration (kernel_stats names krylov_*): CG 3 (krylov_dot, krylov_cg_update, krylov_cg_p), with
 *       LU 4 (a second krylov_dot after the solve); BiCGStab 5 (krylov_dot, krylov_bi_s, krylov_bi_ts, krylov_bi_xr, krylov_bi_p).
 *   res: iters, status (a PEM_KRYLOV_* value), bb, rr (the last residual norm squared the recurrence computed), threshold,
 *       readbacks, launches.  A non-converged status is not an error: the call returns PEM_OK.
 *   pem_krylov_create_amg  (declared with pem_amg_* below) the same solver with PEM_PRECOND_AMG: z = one V-cycle of the hierarchy M,
 *       pem_amg_apply on the solver's stream, where LU runs its two solves -- z is read from an array, every formula above holds with
 *       T replaced by V = pem_amg_info::launches (CG: S = 4 + V, I = 5 + V; BiCGStab: S = 3, I = 7 + 2 V), and the trsv work vector w
 *       is not carved.  opts->precond must be PEM_PRECOND_AMG; M must have been created on the same context and the same A handle
 *       (PEM_E_INVALID otherwise).  The solver holds M as a handle: pem_amg_refresh between solves needs nothing rebuilt; M must outlive
 *       it.  pem_krylov_create itself refuses precond = 3.
 *   Not covered: GMRES and other long-recurrence methods; symmetric Gauss-Seidel and polynomial preconditioners; left
 *       preconditioning; several right-hand sides; graph capture of the iteration; a pem_mgpu_* path; mixed precision beyond the
 *       fp64 scalars. */
enum { PEM_KRYLOV_CG = 0, PEM_KRYLOV_BICGSTAB = 1 };
enum { PEM_PRECOND_NONE = 0, PEM_PRECOND_DIAG = 1, PEM_PRECOND_LU = 2 };
enum { PEM_KRYLOV_CONVERGED = 0, PEM_KRYLOV_MAX_ITERS = 1, PEM_KRYLOV_BREAKDOWN = 2, PEM_KRYLOV_NONFINITE = 3 };
typedef struct {
    int method, precond;
    int64_t max_iters, check_every;
    double rtol, atol;
} pem_krylov_opts;
typedef struct {
    int64_t iters;
    int status;
    double bb, rr, threshold;
    int64_t readbacks, launches;
} pem_krylov_result;
typedef struct pem_krylov pem_krylov;
pem_status pem_krylov_create(pem_ctx *ctx, const pem_tiled *A, const pem_krylov_opts *opts, const pem_tiled *F /* PRECOND_LU, else NULL */,
                             pem_krylov **out);
pem_status pem_krylov_solve(pem_ctx *ctx, pem_krylov *K, const double *db, double *dx /* in: x0, out: x */,
                            const double *d_minv /* PRECOND_DIAG, else NULL */, double *d_history /* max_iters + 1 doubles or NULL */,
                            pem_krylov_result *res);
pem_status pem_krylov_solve_f32(pem_ctx *ctx, pem_krylov *K, const float *db, float *dx, const float *d_minv, double *d_history,
                                pem_krylov_result *res);
pem_status pem_krylov_destroy(pem_ctx *ctx, pem_krylov *K);

/* Aggregation algebraic multigrid: a hierarchy A_0 = A, A_{l+1} = R_l (A_l P_l) built from MIS(2)
 * aggregates, one V-cycle with weighted-Jacobi smoothing as z = M r, and that cycle as the preconditioner of pem_krylov_*.
 *   pem_amg_create  A is square, of either value type VT, with every diagonal entry stored.  THE SETUP IS A SEQUENCE OF PUBLIC
 *       CALLS, so every level is bit for bit what a caller gets by making them.  Level 0 is A itself, held as a handle and not copied
 *       (the rule of plans).  At level l, with n_l rows:
 *         weights    w_i = (VT)omega / d_i, d_i the stored (i, i) value of A_l: omega rounded once to VT, one division.  A row of any
 *                    A_l without a stored diagonal entry is PEM_E_INVALID (the message names the level, the first such row, 1-based,
 *                    and their number).  A stored zero is legal: an infinite weight, and a solver stops on what is not finite
 *                    (NONFINITE, or BREAKDOWN where a dot product is tested first).
 *         stop       level l is the coarsest when l + 1 == max_levels, or n_l <= coarse_size, or the aggregation below returns
 *                    naggregates == n_l (nothing coarsens: a diagonal matrix).
 *         aggregate  pem_tiled_aggregate(A_l, symmetric, seed, NULL).  An entry of -1 (a false symmetric = 1 promise) is
 *                    PEM_E_INVALID; the message says to pass symmetric = 0.
 *         P_t        the n_l x naggregates tiling with a 1 at (v, agg[v]): pem_tiled_from_coo_device of triplets made on the device.
 *         P_l        smooth = 0: P_t.  smooth = 1: T = A_l P_t (pem_cplan_create, pem_spgemm, pem_tiled_from_cplan);
 *                    W = pem_tiled_scale(T, PEM_BINOP_TIMES, d_row = w, NULL); P_l = pem_tiled_ewise(P_t, W, PEM_EWISE_UNION,
 *                    PEM_BINOP_PLUS, alpha = 1, beta = -1) = (I - omega D^-1 A_l) P_t.
 *         A_{l+1}    R_l = pem_tiled_transpose(P_l); AP = A_l P_l; A_{l+1} = R_l AP, each a plan under plus_times with default
 *                    options and pem_tiled_from_cplan.  Structural zeros stay entries, so they are edges of the next aggregation.
 *       All device memory comes from the context's arena; the work vectors of all levels (w and the product vector q per level, x and
 *       b below level 0) are one block.  With refreshable = 0 the plans and T, W, AP (and P_t when smoothed) are destroyed before the
 *       call returns; with refreshable = 1 they are kept for pem_amg_refresh.  Waits.
 *       PEM_E_INVALID, before the device is touched (*out stays NULL): a null argument; rows != cols; smooth, symmetric or refreshable
 *       not 0 / 1; max_levels outside 1 .. PEM_AMG_MAX_LEVELS; coarse_size, sweeps or coarse_sweeps < 1; omega not positive and finite.
 *   pem_amg_refresh  after new values on A (same pattern): the aggregates and every pattern stay.  Level by level: w again, then step 3
 *       of each plan and the matching pem_tiled_set_values_from_cplan / _from_scale / _from_ewise / _from_transpose.  The result
 *       equals a fresh pem_amg_create on the new values, array for array.  Stream-ordered, reads nothing back; the first refresh may
 *       allocate (the refresh maps of ewise and transpose), later ones allocate nothing.  PEM_E_STATE on a hierarchy made with
 *       refreshable = 0.
 *   pem_amg_apply  z = cycle(0) with b_0 = d_r: one V-cycle on A z = r from z = 0.  All arithmetic in VT, one rounding per operation,
 *       no fma in the cycle's own kernels; every A x is pem_tiled_mxv's chain.  cycle(l):
 *         coarsest   x_i = w_i * b_i; then coarse_sweeps - 1 times: q = A_l x; x_i = x_i + w_i * (b_i - q_i).
 *         otherwise  x_i = w_i * b_i; sweeps - 1 such Jacobi sweeps; q = A_l x; r_i = b_i - q_i; b_{l+1} = R_l r (plus_times mxv);
 *                    cycle(l + 1); x = x + P_l x_{l+1} (mxv of P_l with accumulate = 1: the chain starts from the old x_i); sweeps
 *                    Jacobi sweeps.  Pre- and post-smoothing are equal, so the cycle is a symmetric operator for a symmetric A.
 *       No reduction, no atomic; every element is written by the thread that computed it, and no kernel reads at another index an
 *       array its own launch writes: the bits do not depend on the launch shape.  Allocates nothing, never waits, reads nothing back.
 *       PEM_E_INVALID: a null ctx or hierarchy; another context than create's; the fp64 form on an fp32 tiling or the reverse; a null
 *       vector where n > 0; d_r overlapping d_z.  n = 0 is legal and launches nothing.
 *   pem_amg_get_info  levels; rows, nnz of every A_l; p_nnz of every P_l (0 at the coarsest); aggregate_rounds (0 where no aggregation
 *       ran); launches = the kernel launches of ONE pem_amg_apply, the mxv launches included: 2 coarse_sweeps - 1 at the coarsest
 *       level, 4 sweeps + 3 at every other; bytes = what create added to the arena's bytes in use (the hierarchy beyond A itself, and
 *       whatever its calls grew the context's scratch by), as of create's return.
 *   pem_amg_get_level  borrowed handles, valid until pem_amg_destroy: A_l, P_l and R_l = P_l^T as a tiling (P and R NULL at the
 *       coarsest level).  Any of the three pointers may be NULL.
 *   Not covered: strength-of-connection filtering; a spectral-radius estimate for omega; W- and K-cycles; Chebyshev and Gauss-Seidel
 *       smoothers; a direct coarsest solve; graph capture of the cycle; fusing the smoother into the mxv kernel; a pem_mgpu_* path. */
enum { PEM_AMG_MAX_LEVELS = 16 };
typedef struct {
    int      smooth;         /* 0: piecewise-constant P (one 1 per row); 1: Jacobi-smoothed P */
    int      symmetric;      /* handed to pem_tiled_aggregate at every level */
    uint32_t seed;           /* pem_tiled_aggregate's seed, the same at every level; d_priority = NULL */
    int32_t  max_levels;     /* 1 .. PEM_AMG_MAX_LEVELS */
    int64_t  coarse_size;    /* >= 1: a level with n_l <= coarse_size is the coarsest */
    int32_t  sweeps;         /* >= 1: Jacobi sweeps before and after the coarse correction */
    int32_t  coarse_sweeps;  /* >= 1: Jacobi sweeps on the coarsest level */
    double   omega;          /* > 0 and finite: the Jacobi weight, of the smoother and of the smoothed P alike */
    int      refreshable;    /* 1: keep the plans and intermediates pem_amg_refresh needs; 0: free them after setup */
} pem_amg_opts;
typedef struct {
    int32_t levels;
    int64_t rows[PEM_AMG_MAX_LEVELS], nnz[PEM_AMG_MAX_LEVELS];     /* of A_l */
    int64_t p_nnz[PEM_AMG_MAX_LEVELS];                             /* of P_l, 0 at the coarsest */
    int32_t aggregate_rounds[PEM_AMG_MAX_LEVELS];
    int64_t launches;        /* kernel launches of ONE pem_amg_apply, the mxv launches included */
    int64_t bytes;           /* device bytes the object holds beyond A itself */
} pem_amg_info;
typedef struct pem_amg pem_amg;
pem_status pem_amg_create(pem_ctx *ctx, const pem_tiled *A, const pem_amg_opts *opts, pem_amg **out);
pem_status pem_amg_refresh(pem_ctx *ctx, pem_amg *M);
pem_status pem_amg_apply(pem_ctx *ctx, pem_amg *M, const double *d_r, double *d_z);
pem_status pem_amg_apply_f32(pem_ctx *ctx, pem_amg *M, const float *d_r, float *d_z);
pem_status pem_amg_get_info(const pem_amg *M, pem_amg_info *info);
pem_status pem_amg_get_level(const pem_amg *M, int level, const pem_tiled **A_l, const pem_tiled **P_l, const pem_tiled **R_l);
pem_status pem_amg_destroy(pem_ctx *ctx, pem_amg *M);
enum { PEM_PRECOND_AMG = 3 };
pem_status pem_krylov_create_amg(pem_ctx *ctx, const pem_tiled *A, const pem_krylov_opts *opts, const pem_amg *M, pem_krylov **out);

/* A tiling as CSR (host arrays, the calling convention of pem_c_export_csr): rowptr has rows + 1 entries, column indices ascend
 * inside a row, values are copied bit for bit.  Any tiling works; one built with transpose = 1 exports M^T.  rowptr == NULL: only
 * *nnz is set.  The fp64 form refuses an fp32 tiling and vice versa (PEM_E_INVALID).  Waits. */
pem_status pem_tiled_export_csr(pem_ctx *ctx, const pem_tiled *t, int64_t *nnz, int32_t *rowptr, int32_t *colidx, double *vals);
pem_status pem_tiled_export_csr_f32(pem_ctx *ctx, const pem_tiled *t, int64_t *nnz, int32_t *rowptr, int32_t *colidx, float *vals);

/* Plan options.  A new plan takes its defaults from the environment once, in pem_cplan_create (PEM_PRUNE=0, PEM_STEP1=esc,
 * PEM_WIDE=0, PEM_NO_WARM=1, PEM_S3_BAND=0, PEM_EXPORT=rows); after that only pem_cplan_set_option changes them -- no entry
 * point reads the environment at call time.  Changing an option sends the plan back to the last step the option does not touch
 * and makes the next pass a full (size-reading) one.  The values below are the public ones; the test hooks and tuning switches
 * of the kernels (same entry points, further values of pem_option) are declared in pem_test.h. */
typedef enum {
    PEM_OPT_PRUNE = 0,              /* 1 (default): drop tile products whose tiles cannot meet; 0: the reference's lists      */
    PEM_OPT_STEP1_GLOBAL_SORT = 1,  /* 0 (default): row-local LDS sorts; 1: global expand + radix sort (A/B baseline of step 1) */
    PEM_OPT_WIDE = 2,               /* 1 (default): fused step 2 + entry-per-lane step 3; 0: 16-lanes-per-tile baseline kernels */
    PEM_OPT_WARM = 3,               /* 1 (default): repeat passes re-use the previous pass's sizes (device-verified); 0: read back */
    PEM_OPT_S3_BAND = 4,            /* 1 (default): many-pair C tiles of deep plans go to the wave-per-tile kernel              */
    PEM_OPT_EXPORT_ROWS = 7,        /* 0 (default): balanced chunk export; 1: 16 lanes per tile row (A/B baseline)             */
    PEM_OPT__TEST_FIRST = 5,        /* (5, 6, 8-20: pem_test.h)                                                                 */
    PEM_OPT__LAST = 21              /* one past the largest value                                                               */
} pem_option;
pem_status pem_cplan_set_option(pem_cplan *plan, pem_option which, int64_t value);
pem_status pem_cplan_get_option(const pem_cplan *plan, pem_option which, int64_t *value);

/* step 1 (spgemm.cu:1141-1218: tile_spgemm_step1_*_spa_kernel or the NSPARSE symbolic
 * path): tile-level symbolic product -> C tile list sorted by (tile row, tile col).
 * By default products whose A tile's occupied columns miss the B tile's occupied rows are
 * dropped (they contribute nothing; the reference keeps them as empty pairs / empty C tiles).
 * The final C is identical; PEM_OPT_PRUNE = 0 reproduces the reference's lists. */
pem_status pem_spgemm_step1(pem_ctx *ctx, pem_cplan *plan);
/* step 2 (spgemm.cu:1220-1309: search_pairs<0/1>, compute_CMasksAndOffsets,
 * compute_CrowColIdx): pair lists, C tile bitmasks, per-tile nnz, intra-tile CSR. */
pem_status pem_spgemm_step2(pem_ctx *ctx, pem_cplan *plan);
/* step 3 (spgemm.cu:1313-1336: pem_spgemm_step3_accumulate): numeric values. */
pem_status pem_spgemm_step3(pem_ctx *ctx, pem_cplan *plan);
/* steps 1-3 back to back = one iteration of the reference's timed loop (spgemm.cu:1133-1341). */
pem_status pem_spgemm(pem_ctx *ctx, pem_cplan *plan);

typedef struct {
    int32_t tile_row_begin, tile_row_end;
    int32_t row_begin, row_end;    /* matrix rows of C this plan produces */
    int64_t ntiles_c;              /* T_C  (_C_nnz, spgemm.cu:1169)        */
    int64_t npairs;                /* pairs kept: products whose tiles can meet (== npairs_all with PEM_PRUNE=0) */
    int64_t nnz_c;                 /* C_nnz (spgemm.cu:1291)               */
    int64_t npairs_all;            /* P    (d_pairs_count, spgemm.cu:1246): every tile-level product, as the reference counts them */
} pem_cplan_info;
pem_status pem_cplan_get_info(const pem_cplan *plan, pem_cplan_info *info);

typedef enum {
    PEM_C_TILE_ROWPTR = 0,   /* int32[(tr_end-tr_begin)+1] _C_rowPtr            spgemm.cu:1166-1168 */
    PEM_C_TILE_ROWIDX,       /* int32[T_C] absolute tile row                    spgemm.cu:378 */
    PEM_C_TILE_COLIDX,       /* int32[T_C]                                      spgemm.cu:379 */
    PEM_C_PAIRS_OFFSET,      /* int32[T_C+1]                                    spgemm.cu:484, 1242 */
    PEM_C_PAIRS_A,           /* int32[P] A tile id, ascending k inside a C tile spgemm.cu:430 */
    PEM_C_PAIRS_B,           /* int32[P] B tile id                              spgemm.cu:428-431 */
    PEM_C_MASK,              /* uint32[8 T_C] (row 2q)<<16 | row 2q+1           spgemm.cu:533-543 */
    PEM_C_TILE_NNZ_PTR,      /* int32[T_C+1]                                    spgemm.cu:546, 1288 */
    PEM_C_ROWPTR,            /* uint8[16 T_C]                                   spgemm.cu:579-580 */
    PEM_C_ROWCOLIDX,         /* uint8[C_nnz] (on demand where step 3 decodes)   spgemm.cu:582-587 */
    PEM_C_VALS               /* double[C_nnz] (float for an fp32 plan)          spgemm.cu:643-656 */
} pem_cplan_array;
pem_status pem_cplan_get_array(pem_ctx *ctx, const pem_cplan *plan, pem_cplan_array which, void *host_dst, int64_t bytes);

/* Graph replay of repeat passes (off by default; PEM_GRAPH=1 in the environment turns it on at context creation).
 * The reference's timed loop re-launches every kernel of every pass (spgemm.cu:1133-1357).  With replay on, the second
 * and later pem_spgemm calls on an unchanged plan run as ONE hipGraph captured from the first repeat pass (same
 * kernels, grids and buffers: results are identical).  A replayed pass has no per-step events, so pem_timings reports
 * step1/2/3_ms = 0 for it and only spgemm_wall_ms; take the step split from a pass made with replay off. */
pem_status pem_set_graph_replay(pem_ctx *ctx, int on);

/* ---- a14: tiled C -> CSR / sorted COO (spgemm.cu:663-695, 1493-1543) ------------------- */
/* rowptr has (row_end-row_begin)+1 entries and is relative to the slice (rowptr[0] = 0);
 * column indices ascend inside a row.  COO rows are absolute, sorted by (row, col).
 * The _device forms write device arrays and return without waiting for the stream; pem_ctx_synchronize() is where a
 * failure inside their kernels (a device scan that gave up: PEM_E_HIP) is reported.  The host forms wait and report it. */
pem_status pem_c_export_csr(pem_ctx *ctx, const pem_cplan *plan, int64_t *nnz, int32_t *rowptr,
                            int32_t *colidx, double *vals);
pem_status pem_c_export_csr_device(pem_ctx *ctx, const pem_cplan *plan, int32_t *d_rowptr,
                                   int32_t *d_colidx, double *d_vals);
pem_status pem_c_export_coo(pem_ctx *ctx, const pem_cplan *plan, int64_t *nnz, int32_t *rows,
                            int32_t *cols, double *vals);
/* the same for a plan over fp32 tilings */
pem_status pem_c_export_csr_f32(pem_ctx *ctx, const pem_cplan *plan, int64_t *nnz, int32_t *rowptr,
                                int32_t *colidx, float *vals);
pem_status pem_c_export_csr_device_f32(pem_ctx *ctx, const pem_cplan *plan, int32_t *d_rowptr,
                                       int32_t *d_colidx, float *d_vals);
pem_status pem_c_export_coo_f32(pem_ctx *ctx, const pem_cplan *plan, int64_t *nnz, int32_t *rows,
                                int32_t *cols, float *vals);

/* ---- multi-GPU helper: balanced tile-row split (new) ----------------------- */
/* bounds[0..nparts] tile-row boundaries of A, balanced on the per-tile-row intermediate
 * product count (the quantity of spgemm_nsparse_kernel.h:135-151 at tile level). */
pem_status pem_split_tile_rows(pem_ctx *ctx, const pem_tiled *A, const pem_tiled *B, int nparts, int32_t *bounds);
/* weights[0 .. A's tile rows): the per-tile-row weights pem_split_tile_rows balances (tile-level products + tiles + 1), for callers
 * that cut their own row blocks -- e.g. re-cut them from measured per-rank times (multigpu.tune_row_bounds). */
pem_status pem_tile_row_weights(pem_ctx *ctx, const pem_tiled *A, const pem_tiled *B, double *weights);

/* ---- timings (spgemm.cu:1343-1354: the per-step spans of the benchmark CSV) -------------- */
typedef struct {
    double step1_ms, step2_ms, step3_ms;   /* hipEvent spans on the context's stream       */
    double spgemm_wall_ms;                 /* host wall of the last pem_spgemm (CSV col 11)  */
    double export_ms;                      /* last pem_c_export_* device span               */
} pem_timings;
pem_status pem_get_timings(pem_ctx *ctx, pem_timings *t);

/* Per-kernel device time (hipEvent pairs around every launch on the context's stream).
 * Profiling serialises nothing extra but adds two event records per launch; off by default. */
pem_status pem_set_kernel_profiling(pem_ctx *ctx, int enabled);
pem_status pem_reset_kernel_stats(pem_ctx *ctx);
pem_status pem_kernel_stats_count(pem_ctx *ctx, int *n);
pem_status pem_kernel_stats_get(pem_ctx *ctx, int idx, char *name, int name_cap, int64_t *calls, double *total_ms);

#ifdef __cplusplus
}
#endif
#endif
