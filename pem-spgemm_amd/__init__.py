"""pem-spgemm_amd -- host-side Python view of libpemspgemm_hip.so (ctypes over the C ABI).

The product is the HIP library behind include/pem_spgemm.h plus the C++ `pemspgemm` CLI
(host/); this module is the thin binding the tests, bench.py and the multi-GPU driver use.
There is NO CPU fallback: if the shared library is missing or no GPU is visible, every
compute entry point raises.  The directory name carries a hyphen (it mirrors the reference
repo's name), so import it through `__graft_entry__.load_package()`.
"""
import ctypes as C
import numbers
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpemspgemm_hip.so")

PEM_OK = 0
STATUS_NAMES = {0: "PEM_OK", -1: "PEM_E_INVALID", -2: "PEM_E_DUPLICATE", -3: "PEM_E_NOMEM", -4: "PEM_E_OVERFLOW",
                -5: "PEM_E_HIP", -6: "PEM_E_STATE", -7: "PEM_E_NODEVICE", -8: "PEM_E_IO", -9: "PEM_E_STALE"}

# enum pem_tiled_array / pem_cplan_array (include/pem_spgemm.h)
T_ARRAYS = dict(tile_keys=(0, np.int64), tile_nnz_ptr=(1, np.int32), masks=(2, np.uint16), rowptr=(3, np.uint8),
                rowcolidx=(4, np.uint8), vals=(5, np.float64), masks_t=(6, np.uint16), tile_rowptr=(7, np.int32),
                tile_colidx=(8, np.int32), tile_colptr=(9, np.int32), tile_rowidx=(10, np.int32), tile_offsets=(11, np.int32))
C_ARRAYS = dict(c_tile_rowptr=(0, np.int32), c_tile_rowidx=(1, np.int32), c_tile_colidx=(2, np.int32), pairs_offset=(3, np.int32),
                pairs_a=(4, np.int32), pairs_b=(5, np.int32), c_mask=(6, np.uint32), c_tile_nnz_ptr=(7, np.int32),
                c_rowptr=(8, np.uint8), c_rowcolidx=(9, np.uint8), c_vals=(10, np.float64))
# pem_test.h's further pem_cplan_array values (CPlan.array takes them too): of masked plans, M's tile id per C tile
C_TEST_ARRAYS = dict(c_mtile=(11, np.int32))

# enum pem_mask_flags (include/pem_spgemm.h)
MASK_STRUCTURE, MASK_COMPLEMENT = 0, 1

# enum pem_semiring (include/pem_spgemm.h): how step 3 reduces the products of a C entry
SEMIRINGS = dict(plus_times=0, min_plus=1, max_plus=2, max_times=3, plus_pair=4, lor_land=5)

# every symbol include/pem_spgemm.h declares (tests check the library exports all of them)
ABI_SYMBOLS = [
    "pem_last_error", "pem_version", "pem_ctx_create", "pem_ctx_create_on_stream", "pem_ctx_destroy", "pem_ctx_synchronize",
    "pem_tiled_from_coo", "pem_tiled_from_coo_device", "pem_tiled_from_csr", "pem_tiled_destroy", "pem_tiled_get_info",
    "pem_tiled_get_array", "pem_flop_count", "pem_cplan_create", "pem_cplan_destroy", "pem_spgemm_step1", "pem_spgemm_step2",
    "pem_spgemm_step3", "pem_spgemm", "pem_cplan_get_info", "pem_cplan_get_array", "pem_c_export_csr", "pem_c_export_csr_device",
    "pem_c_export_coo", "pem_split_tile_rows", "pem_tile_row_weights", "pem_get_timings", "pem_set_kernel_profiling", "pem_reset_kernel_stats",
    "pem_kernel_stats_count", "pem_kernel_stats_get", "pem_tiled_save", "pem_tiled_load",
    "pem_tiled_from_coo_f32", "pem_tiled_from_coo_device_f32", "pem_tiled_from_csr_f32", "pem_c_export_csr_f32",
    "pem_c_export_csr_device_f32", "pem_c_export_coo_f32", "pem_set_graph_replay",
    "pem_ctx_reserve", "pem_ctx_trim", "pem_ctx_memory_stats", "pem_cplan_set_option", "pem_cplan_get_option", "pem_debug_scan_i32",
    "pem_debug_refused_launch", "pem_tiled_set_values", "pem_tiled_set_values_device", "pem_tiled_set_values_f32",
    "pem_tiled_set_values_device_f32", "pem_cplan_create_masked", "pem_cplan_set_semiring", "pem_cplan_get_semiring",
    "pem_tiled_from_cplan", "pem_tiled_set_values_from_cplan", "pem_tiled_ewise", "pem_tiled_set_values_from_ewise",
    "pem_tiled_export_csr", "pem_tiled_export_csr_f32", "pem_tiled_select", "pem_tiled_set_values_from_select",
    "pem_tiled_mxv", "pem_tiled_mxv_f32", "pem_tiled_reduce", "pem_tiled_reduce_f32", "pem_tiled_spmm", "pem_tiled_spmm_f32",
    "pem_tiled_set_values_sddmm", "pem_tiled_set_values_sddmm_f32", "pem_tiled_sddmm", "pem_tiled_sddmm_f32",
    "pem_tiled_transpose", "pem_tiled_set_values_from_transpose", "pem_tiled_extract", "pem_tiled_extract_device",
    "pem_tiled_set_values_from_extract", "pem_tiled_assign", "pem_tiled_assign_device", "pem_tiled_set_values_from_assign",
    "pem_tiled_mxv_frontier", "pem_tiled_mxv_frontier_f32", "pem_tiled_bfs", "pem_test_frontier_line_flags",
    "pem_tiled_apply", "pem_tiled_set_values_from_apply", "pem_tiled_scale", "pem_tiled_scale_f32", "pem_tiled_set_values_from_scale",
    "pem_tiled_set_values_from_scale_f32", "pem_tiled_kron", "pem_tiled_set_values_from_kron", "pem_tiled_select_topk",
    "pem_tiled_build", "pem_tiled_build_f32", "pem_tiled_build_device", "pem_tiled_build_device_f32", "pem_tiled_set_values_from_build",
    "pem_tiled_set_values_from_build_f32", "pem_tiled_concat", "pem_tiled_set_values_from_concat",
    "pem_tiled_mxv_arg", "pem_tiled_mxv_arg_f32", "pem_tiled_reduce_arg", "pem_tiled_reduce_arg_f32", "pem_tiled_bfs_parents",
    "pem_tiled_sampled_mxm", "pem_tiled_set_values_sampled_mxm",
    "pem_tiled_trsv", "pem_tiled_trsv_f32", "pem_tiled_trsv_info", "pem_test_trsv_split",
    "pem_tiled_ilu0", "pem_tiled_set_values_from_ilu0", "pem_tiled_ilu0_info",
    "pem_tiled_colour", "pem_colour_order", "pem_tiled_components",
    "pem_tiled_mis", "pem_tiled_aggregate",
    "pem_krylov_create", "pem_krylov_solve", "pem_krylov_solve_f32", "pem_krylov_destroy", "pem_test_krylov_dot",
    "pem_amg_create", "pem_amg_refresh", "pem_amg_apply", "pem_amg_apply_f32", "pem_amg_get_info", "pem_amg_get_level", "pem_amg_destroy",
    "pem_krylov_create_amg",
]

# PEM_KRYLOV_CG / _BICGSTAB, PEM_PRECOND_NONE / _DIAG / _LU and the PEM_KRYLOV_* statuses (include/pem_spgemm.h, INTEGRATION.md
# section 3zc), by value
KRYLOV_METHODS = ("cg", "bicgstab")
KRYLOV_PRECONDS = ("none", "diag", "lu")
PRECOND_AMG = 3       # PEM_PRECOND_AMG: through pem_krylov_create_amg only (Krylov.precond then reads "amg")
AMG_MAX_LEVELS = 16   # PEM_AMG_MAX_LEVELS
KRYLOV_STATUS = ("converged", "max_iters", "breakdown", "nonfinite")

# enum pem_ewise_pattern / pem_binop (include/pem_spgemm.h): Tiled.ewise
EWISE_PATTERNS = dict(union=0, intersect=1)
BINOPS = dict(plus=0, times=1, min=2, max=3, lor=4, land=5)
ACCUM_NONE = -1   # PEM_ACCUM_NONE: Tiled.assign without an accum

# Tiled.build's dup operators, by value (include/pem_spgemm.h): the pem_binop values, then PEM_DUP_FIRST and
# PEM_DUP_SECOND; PEM_BUILD_KEEP_MAP; and PEM_BUILD_INORDER_MAX, the longest run of duplicates that is folded strictly left to right
DUP_OPS = ("plus", "times", "min", "max", "lor", "land", "first", "second")
BUILD_KEEP_MAP = 1
BUILD_INORDER_MAX = 32

# enum pem_select_op (include/pem_spgemm.h): Tiled.select's ops, by value; the first eight are positional
SELECT_OPS = ("tril", "triu", "diag", "offdiag", "row_le", "row_gt", "col_le", "col_gt", "value_eq", "value_ne", "value_lt", "value_le",
              "value_gt", "value_ge", "abs_gt")
POSITIONAL_SELECT_OPS = SELECT_OPS[:8]

# enum pem_topk_order (include/pem_spgemm.h): Tiled.select_topk's rank orders, by value
TOPK_ORDERS = ("largest", "smallest", "abs_largest")

# enum pem_apply_op (include/pem_spgemm.h): Tiled.apply's ops, by value; the first six are unary
APPLY_OPS = ("identity", "abs", "ainv", "minv", "sqrt", "one", "plus", "times", "min", "max", "div", "rdiv", "rminus", "powi")

# enum pem_reduce_dim (include/pem_spgemm.h): Tiled.reduce folds every row or every column
REDUCE_DIMS = dict(rows=0, cols=1)

# enum pem_arg_kind (include/pem_spgemm.h): Tiled.mxv_arg's kinds, by value; the last two read no value
ARG_KINDS = ("min_plus", "max_plus", "max_times", "min_index", "max_index")
INDEX_ARG_KINDS = ARG_KINDS[3:]

# PEM_TRSV_LOWER / PEM_TRSV_UPPER (include/pem_spgemm.h): Tiled.trsv's triangles, by value
TRSV_UPLO = ("lower", "upper")

# enum pem_values_order (include/pem_spgemm.h): the order of the values handed to Tiled.set_values*
VALUE_ORDERS = dict(row=0, col=1)

# enum pem_option (include/pem_spgemm.h): kernel variants / test hooks of a plan
OPTIONS = dict(prune=0, step1_global_sort=1, wide=2, warm=3, s3_band=4, s1_force_key64=5, s1_xlcap=6, export_rows=7, s1_serial=8, s3_decode=9, s1_xl_global=10, s3_epw=11, s3_idx64=12, s3_mark=13, s3_xcd=14, s1_segments=15, s2_transposed=16, s3_poison=17,
               s1_class_scan=18, s2_tail_fold=19, s1_one_launch=20, s3_batch=21)


class PemError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {msg}")
        self.status = status


class TiledInfo(C.Structure):
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("nnz", C.c_int64), ("tile_rows", C.c_int32), ("tile_cols", C.c_int32),
                ("ntiles", C.c_int64), ("conv_ms", C.c_double), ("conv_tile_kernel_ms", C.c_double), ("value_bytes", C.c_int32),
                ("reserved", C.c_int32)]


class CPlanInfo(C.Structure):
    _fields_ = [("tile_row_begin", C.c_int32), ("tile_row_end", C.c_int32), ("row_begin", C.c_int32), ("row_end", C.c_int32),
                ("ntiles_c", C.c_int64), ("npairs", C.c_int64), ("nnz_c", C.c_int64), ("npairs_all", C.c_int64)]


class CacheKey(C.Structure):
    """pem_cache_key: what a cached tiling was made from (size + mtime of the source file, transpose flag)."""
    _fields_ = [("source_size", C.c_uint64), ("source_mtime_ns", C.c_int64), ("transpose", C.c_uint32), ("reserved", C.c_uint32)]

    @classmethod
    def of_file(cls, path, transpose=False):
        st = os.stat(path)
        return cls(st.st_size, st.st_mtime_ns, int(bool(transpose)), 0)


class MemoryStats(C.Structure):
    _fields_ = [("slab_bytes", C.c_int64), ("in_use_bytes", C.c_int64), ("peak_in_use_bytes", C.c_int64), ("largest_free_bytes", C.c_int64),
                ("driver_allocs", C.c_int64), ("block_allocs", C.c_int64)]


class TrsvInfo(C.Structure):
    _fields_ = [("levels", C.c_int64), ("launches", C.c_int64), ("max_width", C.c_int64), ("merge_width", C.c_int64),
                ("missing_diag", C.c_int64), ("first_missing_row", C.c_int64)]


class Ilu0Info(C.Structure):
    _fields_ = [("levels", C.c_int64), ("launches", C.c_int64), ("max_width", C.c_int64), ("merge_width", C.c_int64),
                ("zero_pivots", C.c_int64), ("first_zero_pivot_row", C.c_int64)]


class KrylovOpts(C.Structure):
    _fields_ = [("method", C.c_int), ("precond", C.c_int), ("max_iters", C.c_int64), ("check_every", C.c_int64), ("rtol", C.c_double),
                ("atol", C.c_double)]


class KrylovResult(C.Structure):
    _fields_ = [("iters", C.c_int64), ("status", C.c_int), ("bb", C.c_double), ("rr", C.c_double), ("threshold", C.c_double),
                ("readbacks", C.c_int64), ("launches", C.c_int64)]


class AmgOpts(C.Structure):
    _fields_ = [("smooth", C.c_int), ("symmetric", C.c_int), ("seed", C.c_uint32), ("max_levels", C.c_int32), ("coarse_size", C.c_int64),
                ("sweeps", C.c_int32), ("coarse_sweeps", C.c_int32), ("omega", C.c_double), ("refreshable", C.c_int)]


class AmgInfo(C.Structure):
    _fields_ = [("levels", C.c_int32), ("rows", C.c_int64 * AMG_MAX_LEVELS), ("nnz", C.c_int64 * AMG_MAX_LEVELS),
                ("p_nnz", C.c_int64 * AMG_MAX_LEVELS), ("aggregate_rounds", C.c_int32 * AMG_MAX_LEVELS), ("launches", C.c_int64),
                ("bytes", C.c_int64)]


class Timings(C.Structure):
    _fields_ = [("step1_ms", C.c_double), ("step2_ms", C.c_double), ("step3_ms", C.c_double), ("spgemm_wall_ms", C.c_double),
                ("export_ms", C.c_double)]


def build(verbose=False):
    """Compile the HIP library in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    out = None if verbose else subprocess.DEVNULL
    subprocess.check_call(["make", "-C", os.path.join(_HERE, "csrc"), "-j4"], stdout=out)
    return LIB_PATH


_lib = None


def lib():
    """Load libpemspgemm_hip.so; raise (never fall back) when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(the product path has no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        L.pem_last_error.restype = C.c_char_p
        L.pem_version.restype = C.c_char_p
        # (ctx, A, distance, symmetric, seed, d_priority, d_in_set, count, rounds) and
        # (ctx, A, symmetric, seed, d_priority, d_aggregate, d_root, naggregates, rounds): include/pem_spgemm.h
        L.pem_tiled_mis.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64),
                                    C.POINTER(C.c_int32)]
        L.pem_tiled_aggregate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
        L.pem_tiled_mis.restype = L.pem_tiled_aggregate.restype = C.c_int
        # (ctx, A, opts, F, out), (ctx, K, db, dx, d_minv, d_history, res), (ctx, K) and the dot hook (ctx, n, value_bytes, du, dv, out)
        L.pem_krylov_create.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(KrylovOpts), C.c_void_p, C.POINTER(C.c_void_p)]
        L.pem_krylov_solve.argtypes = L.pem_krylov_solve_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                                         C.c_void_p, C.POINTER(KrylovResult)]
        L.pem_krylov_destroy.argtypes = [C.c_void_p, C.c_void_p]
        L.pem_test_krylov_dot.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
        L.pem_krylov_create.restype = L.pem_krylov_solve.restype = L.pem_krylov_solve_f32.restype = C.c_int
        L.pem_krylov_destroy.restype = L.pem_test_krylov_dot.restype = C.c_int
        # (ctx, A, opts, out), (ctx, M), (ctx, M, d_r, d_z), (M, info), (M, level, A_l, P_l, R_l), (ctx, M) and (ctx, A, opts, M, out)
        L.pem_amg_create.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(AmgOpts), C.POINTER(C.c_void_p)]
        L.pem_amg_refresh.argtypes = L.pem_amg_destroy.argtypes = [C.c_void_p, C.c_void_p]
        L.pem_amg_apply.argtypes = L.pem_amg_apply_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.pem_amg_get_info.argtypes = [C.c_void_p, C.POINTER(AmgInfo)]
        L.pem_amg_get_level.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.pem_krylov_create_amg.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(KrylovOpts), C.c_void_p, C.POINTER(C.c_void_p)]
        L.pem_amg_create.restype = L.pem_amg_refresh.restype = L.pem_amg_destroy.restype = L.pem_amg_apply.restype = C.c_int
        L.pem_amg_apply_f32.restype = L.pem_amg_get_info.restype = L.pem_amg_get_level.restype = L.pem_krylov_create_amg.restype = C.c_int
        _lib = L
    return _lib


def _check(status):
    if status != PEM_OK:
        raise PemError(status, lib().pem_last_error().decode(errors="replace"))


def _p(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


class Context:
    """pem_ctx: one per GPU rank (replaces the stream/pool set-up of spgemm.cu:730-758, 808-817)."""

    def __init__(self, device=0, stream=None):
        self._h = C.c_void_p()
        _check(lib().pem_ctx_create_on_stream(int(device), C.c_void_p(stream or 0), C.byref(self._h)))
        self.device = device

    def synchronize(self):
        _check(lib().pem_ctx_synchronize(self._h))

    def timings(self):
        t = Timings()
        _check(lib().pem_get_timings(self._h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in Timings._fields_}

    def reserve(self, nbytes):
        """size the context's device memory arena ahead of time (one driver allocation; the reference sizes its rmm pools
        once, spgemm.cu:808-817)"""
        _check(lib().pem_ctx_reserve(self._h, C.c_int64(int(nbytes))))

    def trim(self):
        """return wholly free slabs of the arena to the driver"""
        _check(lib().pem_ctx_trim(self._h))

    def memory_stats(self):
        m = MemoryStats()
        _check(lib().pem_ctx_memory_stats(self._h, C.byref(m)))
        return {k: getattr(m, k) for k, _ in MemoryStats._fields_}

    def debug_scan(self, values, regime=0, in_place=True, stall_ticket=-1):
        """test hook: the device exclusive scan on a host array -> (prefix sums incl. the closing total, total)"""
        v = np.ascontiguousarray(values, dtype=np.int32)
        out = np.zeros(len(v) + 1, dtype=np.int32)
        total = C.c_int64()
        _check(lib().pem_debug_scan_i32(self._h, _p(v, C.c_int32), C.c_int64(len(v)), int(regime), int(bool(in_place)), int(stall_ticket),
                                        _p(out, C.c_int32), C.byref(total)))
        return out, total.value

    def debug_refused_launch(self):
        """test hook: a kernel launch the runtime refuses; the error surfaces at the next synchronising call"""
        _check(lib().pem_debug_refused_launch(self._h))

    def trsv_split(self, on):
        """test hook (pem_test.h): on forces merge_width = 0 in this context's triangular solves and ILU(0), one launch per level"""
        _check(lib().pem_test_trsv_split(self._h, int(bool(on))))

    def set_graph_replay(self, on):
        """repeat passes of CPlan.spgemm() replayed as one hipGraph (no per-step timings for those passes)"""
        _check(lib().pem_set_graph_replay(self._h, int(bool(on))))

    def set_kernel_profiling(self, on):
        _check(lib().pem_set_kernel_profiling(self._h, int(bool(on))))

    def reset_kernel_stats(self):
        _check(lib().pem_reset_kernel_stats(self._h))

    def kernel_stats(self):
        n = C.c_int()
        _check(lib().pem_kernel_stats_count(self._h, C.byref(n)))
        out = {}
        for i in range(n.value):
            name = C.create_string_buffer(128)
            calls, ms = C.c_int64(), C.c_double()
            _check(lib().pem_kernel_stats_get(self._h, i, name, 128, C.byref(calls), C.byref(ms)))
            out[name.value.decode()] = dict(calls=calls.value, total_ms=ms.value)
        return out

    def close(self):
        if self._h:
            lib().pem_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Tiled:
    """pem_tiled: a matrix in 16x16 tiled-CSR form on the device (spgemm.cu:832-1066)."""

    def __init__(self, ctx, handle, owner=None):
        self.ctx, self._h = ctx, handle
        self._owner = owner   # not None: a view of a handle that object owns (Amg.level); close() then only drops the view
        info = TiledInfo()
        _check(lib().pem_tiled_get_info(self._h, C.byref(info)))
        for k, _ in TiledInfo._fields_:
            setattr(self, k, getattr(info, k))

    @property
    def dtype(self):
        return np.dtype(np.float32 if self.value_bytes == 4 else np.float64)

    @classmethod
    def from_coo(cls, ctx, rows, cols, I, J, V, transpose=False, dtype=np.float64):
        """dtype float64 (the reference's ValueType) or float32 (values are rounded to float here)."""
        f32 = np.dtype(dtype) == np.float32
        I = np.ascontiguousarray(I, dtype=np.int32)
        J = np.ascontiguousarray(J, dtype=np.int32)
        V = np.ascontiguousarray(V, dtype=np.float32 if f32 else np.float64)
        if not (len(I) == len(J) == len(V)):
            raise ValueError("I, J, V lengths differ")
        h = C.c_void_p()
        fn = lib().pem_tiled_from_coo_f32 if f32 else lib().pem_tiled_from_coo
        _check(fn(ctx._h, int(rows), int(cols), C.c_int64(len(I)), _p(I, C.c_int32), _p(J, C.c_int32),
                  _p(V, C.c_float if f32 else C.c_double), int(bool(transpose)), C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def from_coo_device(cls, ctx, rows, cols, nnz, dI, dJ, dV, transpose=False, dtype=np.float64):
        """dI/dJ/dV: device pointers (ints), e.g. torch tensors' data_ptr(); dV points at `dtype` values."""
        h = C.c_void_p()
        fn = lib().pem_tiled_from_coo_device_f32 if np.dtype(dtype) == np.float32 else lib().pem_tiled_from_coo_device
        _check(fn(ctx._h, int(rows), int(cols), C.c_int64(nnz), C.c_void_p(dI), C.c_void_p(dJ), C.c_void_p(dV), int(bool(transpose)),
                  C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def from_csr(cls, ctx, rows, cols, rowptr, colidx, V, dtype=np.float64):
        f32 = np.dtype(dtype) == np.float32
        rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
        colidx = np.ascontiguousarray(colidx, dtype=np.int32)
        V = np.ascontiguousarray(V, dtype=np.float32 if f32 else np.float64)
        h = C.c_void_p()
        fn = lib().pem_tiled_from_csr_f32 if f32 else lib().pem_tiled_from_csr
        _check(fn(ctx._h, int(rows), int(cols), _p(rowptr, C.c_int32), _p(colidx, C.c_int32), _p(V, C.c_float if f32 else C.c_double),
                  C.byref(h)))
        return cls(ctx, h)

    @staticmethod
    def _dup(dup):
        if dup not in DUP_OPS:
            raise ValueError(f"unknown dup op {dup!r}; one of {DUP_OPS}")
        return DUP_OPS.index(dup)

    @classmethod
    def build(cls, ctx, rows, cols, I, J, V, dup="plus", transpose=False, dtype=np.float64, keep_map=False):
        """Build from triplets that may repeat a position: the duplicates of every (row, col) are folded
        on the device in input order, ((v0 op v1) op v2) ..., under dup (one of DUP_OPS; "first" / "second" keep the value that came
        first / last).  The result is an ordinary tiling whose nnz counts the distinct positions.  Runs of at most BUILD_INORDER_MAX
        duplicates are folded strictly left to right.  keep_map=True keeps what set_values_from_build needs.  Waits."""
        dup = cls._dup(dup)
        f32 = np.dtype(dtype) == np.float32
        I = np.ascontiguousarray(I, dtype=np.int32)
        J = np.ascontiguousarray(J, dtype=np.int32)
        V = np.ascontiguousarray(V, dtype=np.float32 if f32 else np.float64)
        if not (len(I) == len(J) == len(V)):
            raise ValueError("I, J, V lengths differ")
        h = C.c_void_p()
        fn = lib().pem_tiled_build_f32 if f32 else lib().pem_tiled_build
        _check(fn(ctx._h, int(rows), int(cols), C.c_int64(len(I)), _p(I, C.c_int32), _p(J, C.c_int32), _p(V, C.c_float if f32 else C.c_double),
                  int(bool(transpose)), dup, BUILD_KEEP_MAP if keep_map else 0, C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def build_device(cls, ctx, rows, cols, nnz_in, dI, dJ, dV, dup="plus", transpose=False, dtype=np.float64, keep_map=False):
        """build from device memory: dI/dJ/dV are device pointers (ints), e.g. torch tensors' data_ptr(), to nnz_in int32 indices and
        `dtype` values, read on the context's stream.  Waits."""
        dup = cls._dup(dup)
        h = C.c_void_p()
        fn = lib().pem_tiled_build_device_f32 if np.dtype(dtype) == np.float32 else lib().pem_tiled_build_device
        _check(fn(ctx._h, int(rows), int(cols), C.c_int64(nnz_in), C.c_void_p(dI), C.c_void_p(dJ), C.c_void_p(dV), int(bool(transpose)),
                  dup, BUILD_KEEP_MAP if keep_map else 0, C.byref(h)))
        return cls(ctx, h)

    def set_values_from_build(self, dV, nnz_in=None):
        """Refresh a tiling made by build(..., keep_map=True) from new values of the same triplet list, in the list's order: the values
        become bit for bit what a fresh build holds.  dV: a contiguous device torch tensor of the tiling's dtype (nnz_in = its length),
        or a device pointer (int) with nnz_in given.  Ordered on the context's stream; returns without waiting."""
        if hasattr(dV, "data_ptr"):
            if not dV.is_cuda or not dV.is_contiguous() or str(dV.dtype) != f"torch.{self.dtype.name}" or nnz_in not in (None, dV.numel()):
                raise ValueError(f"set_values_from_build: want a contiguous device tensor of {self.dtype.name} values, one per triplet, "
                                 f"got {dV.dtype} x {dV.numel()} on {dV.device}")
            nnz_in, dV = dV.numel(), dV.data_ptr()
        if nnz_in is None:
            raise ValueError("set_values_from_build: a device pointer needs nnz_in")
        fn = lib().pem_tiled_set_values_from_build_f32 if self.value_bytes == 4 else lib().pem_tiled_set_values_from_build
        _check(fn(self.ctx._h, self._h, C.c_void_p(int(dV)), C.c_int64(int(nnz_in))))

    def _order(self, order):
        if order not in VALUE_ORDERS:
            raise ValueError(f"order must be one of {sorted(VALUE_ORDERS)}, not {order!r}")
        return VALUE_ORDERS[order]

    def set_values(self, V, order="row"):
        """Numeric refresh: replace the values in place, structure kept (every plan's steps 1-2 stay valid; step 3 recomputes C).
        V: nnz values ordered by (row, col) of the tiled matrix ("row", sorted CSR order) or by (col, row) ("col": for a tiling
        built with transpose=True, the source's CSR order).  Cast to the tiling's dtype as from_coo does; waits."""
        f32 = self.value_bytes == 4
        V = np.ascontiguousarray(V, dtype=self.dtype)
        if V.shape != (self.nnz,):
            raise ValueError(f"set_values: {V.shape} values for a tiling of {self.nnz} entries")
        fn = lib().pem_tiled_set_values_f32 if f32 else lib().pem_tiled_set_values
        _check(fn(self.ctx._h, self._h, _p(V, C.c_float if f32 else C.c_double), self._order(order)))

    def set_values_device(self, dV, order="row"):
        """set_values from device memory, ordered on the context's stream; returns without waiting (errors surface at
        Context.synchronize()).  dV: a device pointer (int) to nnz values of the tiling's dtype, or a torch tensor of them."""
        if hasattr(dV, "data_ptr"):
            if not dV.is_cuda or dV.numel() != self.nnz or not dV.is_contiguous() or str(dV.dtype) != f"torch.{self.dtype.name}":
                raise ValueError(f"set_values_device: want a contiguous device tensor of {self.nnz} {self.dtype.name} values, "
                                 f"got {dV.dtype} x {dV.numel()} on {dV.device}")
            dV = dV.data_ptr()
        fn = lib().pem_tiled_set_values_device_f32 if self.value_bytes == 4 else lib().pem_tiled_set_values_device
        _check(fn(self.ctx._h, self._h, C.c_void_p(int(dV)), self._order(order)))

    @classmethod
    def from_cplan(cls, plan, transpose=False):
        """Chained products: the C of `plan` (or C^T) as a new tiling built on the device, the same
        arrays as from_csr of plan.export_csr(), in C's dtype.  The plan must have run step 3 with current values; the tiling owns its
        arrays and outlives the plan."""
        h = C.c_void_p()
        _check(lib().pem_tiled_from_cplan(plan.ctx._h, plan._h, int(transpose) if transpose in (0, 1) else -1, C.byref(h)))
        return cls(plan.ctx, h)

    def set_values_from_cplan(self, plan):
        """Refresh a tiling made by from_cplan(plan) with the plan's current C values, in place (after the plan's step 3 ran on new
        operand values).  Ordered on the context's stream; returns without waiting."""
        _check(lib().pem_tiled_set_values_from_cplan(self.ctx._h, self._h, plan._h))

    @classmethod
    def ewise(cls, A, B, op="plus", pattern="union", alpha=1.0, beta=1.0):
        """Element-wise combination: a new tiling of A's shape and dtype holding op(alpha*a, beta*b) on the
        union (or intersection) of A's and B's patterns; where only one side is stored (union), that side's scaled value.  op: one of
        BINOPS, pattern: one of EWISE_PATTERNS.  Waits."""
        if op not in BINOPS:
            raise ValueError(f"unknown op {op!r}; one of {sorted(BINOPS)}")
        if pattern not in EWISE_PATTERNS:
            raise ValueError(f"unknown pattern {pattern!r}; one of {sorted(EWISE_PATTERNS)}")
        h = C.c_void_p()
        _check(lib().pem_tiled_ewise(A.ctx._h, A._h, B._h, EWISE_PATTERNS[pattern], BINOPS[op], C.c_double(alpha), C.c_double(beta), C.byref(h)))
        return cls(A.ctx, h)

    def set_values_from_ewise(self, A, B):
        """Refresh a tiling made by ewise(A, B, ...) from A's and B's current values, in place.  Ordered on the context's stream;
        returns without waiting."""
        _check(lib().pem_tiled_set_values_from_ewise(self.ctx._h, self._h, A._h, B._h))

    @classmethod
    def kron(cls, A, B, op="times"):
        """Kronecker product: a new tiling of A.rows * B.rows by A.cols * B.cols in A's dtype that stores
        (i * B.rows + k, j * B.cols + l) with the value op(a_ij, b_kl) wherever A stores (i, j) and B stores (k, l).  op: one of BINOPS
        ("times" is the Kronecker product proper).  A and B may be the same tiling.  Waits."""
        if op not in BINOPS:
            raise ValueError(f"unknown op {op!r}; one of {sorted(BINOPS)}")
        h = C.c_void_p()
        _check(lib().pem_tiled_kron(A.ctx._h, A._h, B._h, BINOPS[op], C.byref(h)))
        return cls(A.ctx, h)

    def set_values_from_kron(self, A, B):
        """Refresh a tiling made by kron(A, B, ...) from A's and B's current values, in place.  Ordered on the context's stream;
        returns without waiting."""
        _check(lib().pem_tiled_set_values_from_kron(self.ctx._h, self._h, A._h, B._h))

    @staticmethod
    def _concat_grid(blocks, row_sizes=None, col_sizes=None):
        """concat's checks, none of which touches the device -> (grid_rows, grid_cols, the blocks row-major, row sizes, column sizes)"""
        if not isinstance(blocks, (list, tuple)) or not blocks or not all(isinstance(row, (list, tuple)) for row in blocks):
            raise ValueError("concat: blocks must be a non-empty list of lists")
        gr, gc = len(blocks), len(blocks[0])
        if gc == 0 or any(len(row) != gc for row in blocks):
            raise ValueError(f"concat: blocks must be rectangular, rows of {[len(row) for row in blocks]} cells are not")
        flat = [b for row in blocks for b in row]
        if not all(b is None or isinstance(b, Tiled) for b in flat):
            raise ValueError("concat: every block must be a Tiled or None")
        some = [b for b in flat if b is not None]
        if not some:
            raise ValueError("concat: every block is None: the result would have no dtype")
        if any(b.value_bytes != some[0].value_bytes for b in some):
            raise ValueError("concat: the blocks hold different dtypes")
        if any(b.ctx is not some[0].ctx for b in some):
            raise ValueError("concat: the blocks belong to different contexts")
        sizes = []
        for name, given, n, dim, line in (("row_sizes", row_sizes, gr, "rows", lambda k: blocks[k]),
                                          ("col_sizes", col_sizes, gc, "cols", lambda k: [row[k] for row in blocks])):
            if given is not None:
                given = [int(x) for x in given]
                if len(given) != n or any(x < 0 for x in given):
                    raise ValueError(f"concat: {name} must hold {n} sizes >= 0, not {given}")
            out = []
            for k in range(n):
                have = sorted({getattr(b, dim) for b in line(k) if b is not None})
                if len(have) > 1:
                    raise ValueError(f"concat: the blocks of grid {dim[:-1]} {k} have {have} {dim}")
                if given is None and not have:
                    raise ValueError(f"concat: grid {dim[:-1]} {k} holds only None: give {name}")
                if given is not None and have and have[0] != given[k]:
                    raise ValueError(f"concat: {name}[{k}] = {given[k]}, but a block there has {have[0]} {dim}")
                out.append(given[k] if given is not None else have[0])
            sizes.append(out)
        return gr, gc, flat, sizes[0], sizes[1]

    @classmethod
    def concat(cls, blocks, row_sizes=None, col_sizes=None):
        """Concat: the block matrix [[B00, B01, ..], [B10, ..], ..] as a new tiling built on the device.
        blocks: a rectangular list of lists of Tiled or None (an all-empty block); the blocks of one grid row have the same rows, of
        one grid column the same cols, and all one dtype.  row_sizes / col_sizes default to the sizes of the non-null blocks of each
        grid row / column; a strip of only None needs its size given (0 is allowed).  The result stores (ro_a + i, co_b + j) where
        block (a, b) stores (i, j), values copied bit for bit.  The same tiling may sit in several cells.  ValueError (before the
        device is touched) for a ragged grid, a size that cannot be determined or contradicts a block, mixed dtypes.  Waits."""
        gr, gc, flat, rs, cs = cls._concat_grid(blocks, row_sizes, col_sizes)
        ctx = next(b for b in flat if b is not None).ctx
        hs = (C.c_void_p * len(flat))(*[None if b is None else b._h for b in flat])
        h = C.c_void_p()
        _check(lib().pem_tiled_concat(ctx._h, gr, gc, hs, (C.c_int64 * gr)(*rs), (C.c_int64 * gc)(*cs), C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def hstack(cls, blocks):
        """[B0 B1 ..]: concat of one grid row"""
        return cls.concat([list(blocks)])

    @classmethod
    def vstack(cls, blocks):
        """[B0; B1; ..]: concat of one grid column"""
        return cls.concat([[b] for b in blocks])

    def set_values_from_concat(self, blocks):
        """Refresh a tiling made by concat(blocks, ...) from the blocks' current values, in place: the same grid again (a list of
        lists), None where the build had None.  Ordered on the context's stream; returns without waiting."""
        flat = [b for row in blocks for b in row]
        hs = (C.c_void_p * max(len(flat), 1))(*[None if b is None else b._h for b in flat])
        _check(lib().pem_tiled_set_values_from_concat(self.ctx._h, self._h, len(flat), hs))

    def split(self, row_sizes, col_sizes):
        """The inverse of concat: a list of lists of new tilings, piece (a, b) = rows ro_a .. ro_a + row_sizes[a] - 1 and columns
        co_b .. co_b + col_sizes[b] - 1 of this one.  Built on extract with slices -- one extract per piece, no kernel of its own.
        The sizes are integers >= 1 (a tiling has at least one row and one column) and sum to the shape.  Waits."""
        rs, cs = [int(x) for x in row_sizes], [int(x) for x in col_sizes]
        for name, s, dim in (("row_sizes", rs, self.rows), ("col_sizes", cs, self.cols)):
            if not s or any(x < 1 for x in s) or sum(s) != dim:
                raise ValueError(f"split: {name} must be sizes >= 1 that sum to {dim}, not {s}")
        ro, co = np.concatenate([[0], np.cumsum(rs)]), np.concatenate([[0], np.cumsum(cs)])
        return [[self.extract(slice(int(ro[a]), int(ro[a + 1])), slice(int(co[b]), int(co[b + 1]))) for b in range(len(cs))]
                for a in range(len(rs))]

    def select(self, op, thunk=0):
        """Select: a new tiling of this one's shape and dtype holding exactly the stored entries that satisfy
        op (one of SELECT_OPS) with the thunk -- an integer k for the positional ops, a value (rounded to the dtype) for the value ops.
        Values are copied bit for bit.  Waits."""
        if op not in SELECT_OPS:
            raise ValueError(f"unknown select op {op!r}; one of {SELECT_OPS}")
        h = C.c_void_p()
        _check(lib().pem_tiled_select(self.ctx._h, self._h, SELECT_OPS.index(op), C.c_double(float(thunk)), C.byref(h)))
        return Tiled(self.ctx, h)

    def set_values_from_select(self, A):
        """Refresh a tiling made by A.select(op, k) with a positional op from A's current values, in place.  Ordered on the context's
        stream; returns without waiting."""
        _check(lib().pem_tiled_set_values_from_select(self.ctx._h, self._h, A._h))

    def select_topk(self, k, order="largest", dim="rows"):
        """Select top-k: a new tiling of this one's shape and dtype holding, of every row (dim "rows") or
        column ("cols"), the first min(k, entries of the line) entries in rank order -- order one of TOPK_ORDERS; NaNs rank last, equal
        entries by ascending index inside the line.  Values are copied bit for bit.  Waits.  There is no refresh: select again."""
        if order not in TOPK_ORDERS:
            raise ValueError(f"unknown top-k order {order!r}; one of {TOPK_ORDERS}")
        if dim not in REDUCE_DIMS:
            raise ValueError(f"unknown dim {dim!r}; one of {sorted(REDUCE_DIMS)}")
        if isinstance(k, bool) or not isinstance(k, numbers.Real) or k != k or k < 0 or k >= 2 ** 63 or int(k) != k:
            raise ValueError(f"k must be an integer >= 0 (below 2^63), not {k!r}")
        h = C.c_void_p()
        _check(lib().pem_tiled_select_topk(self.ctx._h, self._h, TOPK_ORDERS.index(order), REDUCE_DIMS[dim], C.c_int64(int(k)), C.byref(h)))
        return Tiled(self.ctx, h)

    def apply(self, op, thunk=0):
        """Apply: a new tiling of this one's pattern, shape and dtype whose values are op (one of APPLY_OPS)
        of this one's -- unary (identity, abs, ainv, minv, sqrt, one), bound to the thunk rounded to the dtype (plus, times, min, max,
        div, rdiv, rminus) or x^k for an integer k = thunk in 1..64 (powi).  Nothing is dropped: zeros, inf and NaN stay entries.
        Waits."""
        if op not in APPLY_OPS:
            raise ValueError(f"unknown apply op {op!r}; one of {APPLY_OPS}")
        h = C.c_void_p()
        _check(lib().pem_tiled_apply(self.ctx._h, self._h, APPLY_OPS.index(op), C.c_double(float(thunk)), C.byref(h)))
        return Tiled(self.ctx, h)

    def set_values_from_apply(self, A):
        """Refresh a tiling made by A.apply(op, thunk) from A's current values, in place.  Ordered on the context's stream; returns
        without waiting and allocates nothing."""
        _check(lib().pem_tiled_set_values_from_apply(self.ctx._h, self._h, A._h))

    def _scale_vectors(self, fn, rows, cols):
        return (None if rows is None else self._vector(fn, "rows", rows, self.rows),
                None if cols is None else self._vector(fn, "cols", cols, self.cols))

    def scale(self, rows=None, cols=None, op="times"):
        """Scale: a new tiling of this one's pattern, shape and dtype with the values
        op(op(rows[i], a_ij), cols[j]), op one of BINOPS -- "times" is D_r A D_c, "plus" a_ij + h_i + g_j.  rows, cols: contiguous
        device torch tensors of the tiling's dtype with exactly self.rows / self.cols entries, or None: that step is then not
        performed.  Waits."""
        if op not in BINOPS:
            raise ValueError(f"unknown scale op {op!r}; one of {sorted(BINOPS)}")
        pr, pc = self._scale_vectors("scale", rows, cols)
        fn = lib().pem_tiled_scale_f32 if self.value_bytes == 4 else lib().pem_tiled_scale
        h = C.c_void_p()
        _check(fn(self.ctx._h, self._h, BINOPS[op], pr, pc, C.byref(h)))
        return Tiled(self.ctx, h)

    def set_values_from_scale(self, A, rows=None, cols=None):
        """Refresh a tiling made by A.scale(..., op) from A's current values and these vectors (either may be None, whatever the
        build had), in place.  Ordered on the context's stream; returns without waiting and allocates nothing."""
        pr, pc = self._scale_vectors("set_values_from_scale", rows, cols)
        fn = lib().pem_tiled_set_values_from_scale_f32 if self.value_bytes == 4 else lib().pem_tiled_set_values_from_scale
        _check(fn(self.ctx._h, self._h, A._h, pr, pc))

    def _index_list(self, name, L, dim, what="extract"):
        """one argument of extract or assign -> (kind, list, n): kind None (all), "host" (a C-contiguous int32 array) or "device" (a torch
        int32 tensor on the context's device)"""
        if L is None:
            return None, None, 0
        if isinstance(L, slice):
            L = np.arange(*L.indices(dim), dtype=np.int32)
        if hasattr(L, "data_ptr"):
            if L.is_cuda:
                dev = L.device.index if L.device.index is not None else 0
                if str(L.dtype) != "torch.int32" or L.dim() != 1 or not L.is_contiguous() or dev != self.ctx.device:
                    raise ValueError(f"{what}: want a contiguous 1-d int32 tensor on device {self.ctx.device} for {name}, "
                                     f"got {L.dtype} {tuple(L.shape)} on {L.device}")
                return "device", L, L.numel()
            L = L.numpy()
        a = np.asarray(L)
        if a.ndim != 1:
            raise ValueError(f"{what}: {name} must be one-dimensional, not {a.shape}")
        if a.size and a.dtype.kind not in "iu":
            raise ValueError(f"{what}: {name} must hold integers, not {a.dtype}")
        if a.size and (int(a.min()) < 0 or int(a.max()) >= dim):
            raise ValueError(f"{what}: {name} holds an index outside 0 .. {dim - 1} (negative indices are not wrapped)")
        return "host", np.ascontiguousarray(a, dtype=np.int32), a.size

    def extract(self, rows=None, cols=None):
        """Extract: R = A(rows, cols) as a new tiling of this one's dtype; R stores (p, q) where this
        tiling stores (rows[p], cols[q]), values copied bit for bit.  Each argument: None (all, in order), a slice, a host integer
        array-like (checked; negative indices are refused, not wrapped) or a torch int32 tensor on the context's device.  Lists may be
        in any order and may repeat indices (scipy's A[rows][:, cols]).  Waits."""
        kr, I, ni = self._index_list("rows", rows, self.rows)
        kc, J, nj = self._index_list("cols", cols, self.cols)
        device = "device" in (kr, kc)
        if device:   # one device and one host list: upload the host one
            import torch
            dev = torch.device("cuda", self.ctx.device)
            if kr == "host":
                I = torch.from_numpy(I).to(dev)
            if kc == "host":
                J = torch.from_numpy(J).to(dev)
            torch.cuda.current_stream(dev).synchronize()   # (the lists are read on the context's stream)
            # (an empty tensor has a null pointer, which would mean "all": any non-null one lets the library refuse n = 0)
            pI, pJ = (None if x is None else C.c_void_p(x.data_ptr() or 1) for x in (I, J))
            fn = lib().pem_tiled_extract_device
        else:
            pI, pJ = (None if x is None else _p(x, C.c_int32) for x in (I, J))
            fn = lib().pem_tiled_extract
        h = C.c_void_p()
        _check(fn(self.ctx._h, self._h, pI, C.c_int64(ni), pJ, C.c_int64(nj), C.byref(h)))
        return Tiled(self.ctx, h)

    def set_values_from_extract(self, A):
        """Refresh a tiling made by A.extract(rows, cols) from A's current values, in place.  Ordered on the context's stream; returns
        without waiting."""
        _check(lib().pem_tiled_set_values_from_extract(self.ctx._h, self._h, A._h))

    def assign(self, A, rows=None, cols=None, accum=None):
        """Assign: Z = this tiling (C) with Z(rows, cols) = A, or with accum (one of BINOPS)
        Z(rows, cols) = accum(C(rows, cols), A), as a new tiling of C's shape and dtype; C and A are not changed.  Without an accum C's
        entries in the region that A does not store are deleted.  rows, cols: as for extract -- None (all, in order), a slice, a host
        integer array-like (checked: a negative index or a repeat raises ValueError) or a torch int32 tensor on the context's device
        (checked by the library).  A is len(rows) x len(cols).  Waits."""
        if accum is not None and accum not in BINOPS:
            raise ValueError(f"unknown accum {accum!r}; None or one of {sorted(BINOPS)}")
        kr, I, ni = self._index_list("rows", rows, self.rows, "assign")
        kc, J, nj = self._index_list("cols", cols, self.cols, "assign")
        for k, L, name in ((kr, I, "rows"), (kc, J, "cols")):
            if k == "host" and len(np.unique(L)) != len(L):
                raise ValueError(f"assign: {name} repeats an index")
        if "device" in (kr, kc):   # one device and one host list: upload the host one
            import torch
            dev = torch.device("cuda", self.ctx.device)
            if kr == "host":
                I = torch.from_numpy(I).to(dev)
            if kc == "host":
                J = torch.from_numpy(J).to(dev)
            torch.cuda.current_stream(dev).synchronize()   # (the lists are read on the context's stream)
            pI, pJ = (None if x is None else C.c_void_p(x.data_ptr() or 1) for x in (I, J))
            fn = lib().pem_tiled_assign_device
        else:
            pI, pJ = (None if x is None else _p(x, C.c_int32) for x in (I, J))
            fn = lib().pem_tiled_assign
        h = C.c_void_p()
        _check(fn(self.ctx._h, self._h, A._h, pI, C.c_int64(ni), pJ, C.c_int64(nj), ACCUM_NONE if accum is None else BINOPS[accum], C.byref(h)))
        return Tiled(self.ctx, h)

    def set_values_from_assign(self, C_, A):
        """Refresh a tiling made by C_.assign(A, rows, cols, accum) from C_'s and A's current values, in place.  Ordered on the
        context's stream; returns without waiting."""
        _check(lib().pem_tiled_set_values_from_assign(self.ctx._h, self._h, C_._h, A._h))

    def transpose(self):
        """Transpose: this tiling's matrix transposed, as a new tiling built on the device -- the arrays
        of from_coo(.., transpose=True) of the exported entries.  Waits."""
        h = C.c_void_p()
        _check(lib().pem_tiled_transpose(self.ctx._h, self._h, C.byref(h)))
        return Tiled(self.ctx, h)

    def set_values_from_transpose(self, A):
        """Refresh a tiling made by A.transpose() from A's current values, in place.  Ordered on the context's stream; returns without
        waiting."""
        _check(lib().pem_tiled_set_values_from_transpose(self.ctx._h, self._h, A._h))

    def _vector(self, fn, name, v, n):
        """the device pointer of a torch tensor of n values of this tiling's dtype (the check of set_values_device)"""
        if not hasattr(v, "data_ptr") or not v.is_cuda or v.numel() != n or not v.is_contiguous() or str(v.dtype) != f"torch.{self.dtype.name}":
            got = f"{v.dtype} x {v.numel()} on {v.device}" if hasattr(v, "data_ptr") else type(v).__name__
            raise ValueError(f"{fn}: want a contiguous device tensor of {n} {self.dtype.name} values for {name}, got {got}")
        return C.c_void_p(v.data_ptr())

    def _out(self, fn, out, n, like=None):
        if out is None:
            import torch
            dev = like.device if like is not None else torch.device("cuda", self.ctx.device)
            out = torch.empty(n, dtype=getattr(torch, self.dtype.name), device=dev)
        return out, self._vector(fn, "out", out, n)

    def mxv(self, x, semiring="plus_times", transpose=False, out=None, accumulate=False):
        """Matrix-vector product: out = A (+).(x) x, or A^T (+).(x) x with transpose=True, under a
        semiring of SEMIRINGS.  x: a contiguous device torch tensor of the tiling's dtype with cols (transpose: rows) entries; out: one
        with rows (transpose: cols) entries, allocated when None.  Every output is the fold of its row's (column's) entries in
        ascending index -- under plus_times the fma chain, bit for bit what CPlan(A, X) computes -- from the semiring's start value, or
        from out's old value with accumulate=True (empty rows then stay as they are).  x and out must not overlap.  Ordered on the
        context's stream and never waits: on a context created on the torch stream torch works on (s = torch.cuda.Stream(), Context(dev,
        stream=s.cuda_stream), torch.cuda.set_stream(s) -- torch's default stream is the null stream, and stream=None gives the context
        a stream of its own) torch reads out, and may write x, with no extra sync.  Returns out."""
        if semiring not in SEMIRINGS:
            raise ValueError(f"unknown semiring {semiring!r}; one of {sorted(SEMIRINGS)}")
        nx, ny = (self.rows, self.cols) if transpose else (self.cols, self.rows)
        px = self._vector("mxv", "x", x, nx)
        out, py = self._out("mxv", out, ny, like=x)
        fn = lib().pem_tiled_mxv_f32 if self.value_bytes == 4 else lib().pem_tiled_mxv
        _check(fn(self.ctx._h, self._h, SEMIRINGS[semiring], int(bool(transpose)), px, py, int(bool(accumulate))))
        return out

    def trsv(self, b, uplo="lower", unit_diag=False, out=None):
        """Triangular solve: out = T^-1 b, T the lower or upper triangle (uplo, one of TRSV_UPLO) of this
        square tiling as stored -- entries on the other side are ignored, and with unit_diag=True so are the stored diagonal entries
        (the diagonal counts as 1).  b: a contiguous device torch tensor of the tiling's dtype with rows entries; out: one like it,
        allocated when None; out is b solves in place.  Any other argument raises ValueError; what the library refuses (a partial overlap,
        a tiling that is not square) raises PemError.  Bit-exact order: section 3x.  A row without a
        stored diagonal entry is refused unless unit_diag.  The first call per triangle builds the level schedule (waits once); every
        later call is ordered on the context's stream and never waits (see mxv).  Returns out."""
        if uplo not in TRSV_UPLO:
            raise ValueError(f"unknown uplo {uplo!r}; one of {TRSV_UPLO}")
        pb = self._vector("trsv", "b", b, self.rows)
        out, px = self._out("trsv", out, self.rows, like=b)
        fn = lib().pem_tiled_trsv_f32 if self.value_bytes == 4 else lib().pem_tiled_trsv
        _check(fn(self.ctx._h, self._h, TRSV_UPLO.index(uplo), int(bool(unit_diag)), pb, px))
        return out

    def trsv_info(self, uplo="lower"):
        """the schedule of a triangle (built if need be) as a dict: levels, launches (of one solve), max_width (tile rows of the
        widest level), merge_width, missing_diag (rows without a stored diagonal entry), first_missing_row (1-based, 0 if none)"""
        if uplo not in TRSV_UPLO:
            raise ValueError(f"unknown uplo {uplo!r}; one of {TRSV_UPLO}")
        i = TrsvInfo()
        _check(lib().pem_tiled_trsv_info(self.ctx._h, self._h, TRSV_UPLO.index(uplo), C.byref(i)))
        return {k: int(getattr(i, k)) for k, _ in TrsvInfo._fields_}

    def ilu0(self):
        """ILU(0): the incomplete LU of this square tiling on its own pattern as a new tiling F of the same
        pattern and dtype -- L's strict lower triangle (unit diagonal, not stored) and U with its diagonal.  Bit-exact order: section
        3y.  Every row must store its diagonal entry (PemError names the first that does not).  Waits."""
        h = C.c_void_p()
        _check(lib().pem_tiled_ilu0(self.ctx._h, self._h, C.byref(h)))
        return Tiled(self.ctx, h)

    def set_values_from_ilu0(self, A):
        """Refresh a tiling made by A.ilu0() from A's current values, in place: bit for bit a fresh A.ilu0().  Ordered on the context's
        stream; returns without waiting and allocates nothing."""
        _check(lib().pem_tiled_set_values_from_ilu0(self.ctx._h, self._h, A._h))

    def ilu0_info(self):
        """of a factor: levels, launches, max_width and merge_width of the factorisation's launch plan, zero_pivots (rows whose f_ii is
        +-0, not finite or not stored) and first_zero_pivot_row (1-based, 0 if none), as a dict.  Waits."""
        i = Ilu0Info()
        _check(lib().pem_tiled_ilu0_info(self.ctx._h, self._h, C.byref(i)))
        return {k: int(getattr(i, k)) for k, _ in Ilu0Info._fields_}

    def colour(self, seed=0, priority=None, symmetric=False, out=None):
        """Greedy colouring of this square tiling's pattern: every stored off-diagonal (i, j) is an
        undirected edge, values are never read.  Returns (colours, ncolours, rounds): colours an int32 device torch tensor (out,
        written in place, when given) with colours[v] the smallest colour no neighbour of higher priority holds.  The priority of v is
        a hash of v and seed (an integer in [0, 2^32)), or priority[v] -- a contiguous uint32 / int32 (read as uint32) torch tensor on
        the context's device, or a host array of integers in [0, 2^32), uploaded -- larger first, ties to the lower index: equal
        priorities give the natural-order greedy colouring.  symmetric=True promises a symmetric pattern (only the rows are walked;
        the same result there).  Fully determined: two calls give identical tensors.  Waits (one small read-back per round)."""
        seed = _colour_seed(seed)
        priority, pp = self._priority_arg("colour", priority)
        out, pc = self._index_out("colour", "out", out, self.rows)
        ncolours, rounds = C.c_int32(), C.c_int32()
        _check(lib().pem_tiled_colour(self.ctx._h, self._h, int(bool(symmetric)), C.c_uint32(seed), pp, pc, C.byref(ncolours), C.byref(rounds)))
        return out, ncolours.value, rounds.value

    def _priority_arg(self, fn, priority):
        """(tensor kept alive, device pointer or None) of colour's / mis' / aggregate's priority: a device tensor as it is, a host
        array uploaded"""
        if priority is None:
            return None, None
        import torch
        dev = torch.device("cuda", self.ctx.device)
        if hasattr(priority, "data_ptr"):
            if (not priority.is_cuda or priority.device.index != self.ctx.device or priority.dim() != 1 or priority.numel() != self.rows
                    or not priority.is_contiguous() or str(priority.dtype) not in ("torch.int32", "torch.uint32")):
                raise ValueError(f"{fn}: want a contiguous device tensor of {self.rows} uint32 or int32 values on cuda:{self.ctx.device} "
                                 f"for priority, got {priority.dtype} of shape {tuple(priority.shape)} on {priority.device}")
        else:
            priority = torch.from_numpy(_colour_priority(priority, self.rows, fn).view(np.int32)).to(dev)
            torch.cuda.current_stream(dev).synchronize()   # (the priorities are read on the context's stream)
        return priority, C.c_void_p(priority.data_ptr() or 1)

    def mis(self, distance=2, seed=0, priority=None, symmetric=False, out=None):
        """Maximal independent set at distance 1 or 2 of this square tiling's pattern: the graph, seed,
        priority and symmetric are colour's.  Returns (in_set, count, rounds): in_set a torch.uint8 device tensor of 0 / 1 (out,
        written in place, when given) -- the set the sequential greedy pass in "beats" order builds: v enters iff no vertex already
        in the set lies within `distance` of it; count its size; rounds the rounds the device ran.  Fully determined: two calls give
        identical tensors.  Waits (one small read-back per round)."""
        if isinstance(distance, bool) or distance not in (1, 2):
            raise ValueError(f"mis: distance must be 1 or 2, not {distance!r}")
        seed = _colour_seed(seed, "mis")
        import torch
        priority, pp = self._priority_arg("mis", priority)
        if out is None:
            out = torch.empty(self.rows, dtype=torch.uint8, device=torch.device("cuda", self.ctx.device))
        if (not hasattr(out, "data_ptr") or not out.is_cuda or out.device.index != self.ctx.device or out.numel() != self.rows
                or out.dim() != 1 or not out.is_contiguous() or out.dtype != torch.uint8):
            got = f"{out.dtype} of shape {tuple(out.shape)} on {out.device}" if hasattr(out, "data_ptr") else type(out).__name__
            raise ValueError(f"mis: want a contiguous device tensor of {self.rows} uint8 values on cuda:{self.ctx.device} for out, got {got}")
        count, rounds = C.c_int64(), C.c_int32()
        _check(lib().pem_tiled_mis(self.ctx._h, self._h, int(distance), int(bool(symmetric)), C.c_uint32(seed), pp,
                                   C.c_void_p(out.data_ptr() or 1), C.byref(count), C.byref(rounds)))
        return out, count.value, rounds.value

    def aggregate(self, seed=0, priority=None, symmetric=False, out=None, roots=True):
        """MIS(2) aggregation of this square tiling's pattern: the roots are self.mis(2, ...), numbered
        in ascending vertex order; a root's neighbours join it, then every vertex still free joins the aggregate of the placed
        neighbour that beats the others.  Returns (agg, roots, naggregates, rounds): agg an int32 device tensor (out, written in
        place, when given) with agg[v] in [0, naggregates); roots the int32 device tensor of naggregates root vertices, or None with
        roots=False (the library then gets NULL); rounds those of the set.  Under a false symmetric=True promise agg may hold -1.
        Fully determined.  Waits (one small read-back per round)."""
        seed = _colour_seed(seed, "aggregate")
        priority, pp = self._priority_arg("aggregate", priority)
        out, pa = self._index_out("aggregate", "out", out, self.rows)
        root_t, pr = (self._index_out("aggregate", "roots", None, self.rows) if roots else (None, None))
        nagg, rounds = C.c_int64(), C.c_int32()
        _check(lib().pem_tiled_aggregate(self.ctx._h, self._h, int(bool(symmetric)), C.c_uint32(seed), pp, pa, pr, C.byref(nagg),
                                         C.byref(rounds)))
        return out, (root_t[:nagg.value] if roots else None), nagg.value, rounds.value

    def reorder_by_colour(self, seed=0, symmetric=False):
        """The colour reordering: (R, perm, offsets) with perm, offsets = colour_order of self.colour(seed,
        symmetric=symmetric) and R = self.extract(perm, perm) -- inside a colour no vertex waits for another, so R.trsv and R.ilu0 have
        few levels.  Composed from colour, colour_order and extract: R.set_values_from_extract(self) refreshes R.  Waits."""
        colours, ncolours, _ = self.colour(seed=seed, symmetric=symmetric)
        perm, offsets = colour_order(self.ctx, colours, ncolours)
        return self.extract(perm, perm), perm, offsets

    def components(self, symmetric=False, out=None, ids=True, out_ids=None):
        """Connected components of this square tiling's pattern: every stored entry (i, j) is the
        undirected edge {i, j}, values are never read.  Returns (labels, ids, ncomponents, rounds): labels an int32 device torch
        tensor (out, written in place, when given) with labels[v] the smallest vertex of v's component; ids likewise (out_ids) the
        dense component ids 0 .. ncomponents - 1 in order of smallest vertex, or None with ids=False (the library then gets NULL);
        rounds the rounds of the label propagation, the last one, which changes nothing, included.  symmetric=True promises a
        symmetric pattern (only the rows are walked; the same result there; on another pattern 0 <= labels[v] <= v and nothing
        more).  Fully determined: two calls give identical tensors.  Waits (one small read-back per round)."""
        if not ids and out_ids is not None:
            raise ValueError("components: out_ids given with ids=False")
        out, pl = self._index_out("components", "out", out, self.rows)
        pi = None
        if ids:
            out_ids, pi = self._index_out("components", "out_ids", out_ids, self.rows)
        ncomponents, rounds = C.c_int64(), C.c_int32()
        _check(lib().pem_tiled_components(self.ctx._h, self._h, int(bool(symmetric)), pl, pi, C.byref(ncomponents), C.byref(rounds)))
        return out, (out_ids if ids else None), ncomponents.value, rounds.value

    def reorder_by_component(self, symmetric=False):
        """The component reordering: (R, perm, offsets) with perm, offsets = colour_order of the ids of
        self.components(symmetric=symmetric) and R = self.extract(perm, perm) -- block diagonal, the blocks in order of their
        smallest vertex, the vertices ascending inside a block; block c is R.extract(slice(offsets[c], offsets[c + 1]), the same).
        Composed from components, colour_order and extract: R.set_values_from_extract(self) refreshes R.  Waits."""
        _, ids, ncomponents, _ = self.components(symmetric=symmetric)
        perm, offsets = colour_order(self.ctx, ids, ncomponents)
        return self.extract(perm, perm), perm, offsets

    def lu_solve(self, b, out=None, work=None):
        """z = U^-1 L^-1 b with this tiling an ILU(0) factor: trsv(b, "lower", unit_diag=True, out=work), then trsv(work, "upper",
        out=out).  b, out, work: as trsv's vectors; out and work are allocated when None.  Never waits once both schedules exist.
        Returns out."""
        work = self.trsv(b, "lower", unit_diag=True, out=work)
        return self.trsv(work, "upper", out=out)

    def solve(self, b, method="cg", precond=None, x=None, max_iters=1000, check_every=8, rtol=1e-8, atol=0.0, history=False):
        """A x = b in one call: makes a Krylov solver, solves, closes it; returns (x, info) as
        Krylov.solve.  precond: None, "jacobi" (minv = 1 / self.select("diag", 0).reduce("plus"), the DIAG preconditioner), "ilu0"
        (makes and closes its own factor), "amg" (makes and closes its own default Amg), a tiling (an LU factor), an Amg made on this
        tiling, or a device tensor (minv itself)."""
        minv, F, own = None, None, None
        if isinstance(precond, str):
            if precond == "jacobi":
                D = self.select("diag", 0)
                try:
                    minv = 1 / D.reduce("plus")
                finally:
                    D.close()
                import torch
                torch.cuda.current_stream(minv.device).synchronize()   # (torch's division; minv is read on the context's stream)
                precond = "diag"
            elif precond == "ilu0":
                precond = own = self.ilu0()
            elif precond == "amg":
                precond = own = Amg(self)
            elif precond != "none":
                raise ValueError(f"solve: unknown precond {precond!r}; None, 'none', 'jacobi', 'ilu0', 'amg', a tiling, an Amg or a device "
                                 "tensor")
        elif hasattr(precond, "data_ptr"):
            minv, precond = precond, "diag"
        try:
            K = Krylov(self, method=method, precond=precond, max_iters=max_iters, check_every=check_every, rtol=rtol, atol=atol)
            try:
                return K.solve(b, x=x, minv=minv, history=history)
            finally:
                K.close()
        finally:
            if own is not None:
                own.close()

    def _bytes(self, fn, name, v, n):
        """the device pointer of a contiguous torch.bool / torch.uint8 tensor of n bytes on the context's device; None passes as NULL"""
        if v is None:
            return None
        if (not hasattr(v, "data_ptr") or not v.is_cuda or v.device.index != self.ctx.device or v.numel() != n or v.dim() != 1
                or not v.is_contiguous() or str(v.dtype) not in ("torch.bool", "torch.uint8")):
            got = f"{v.dtype} of shape {tuple(v.shape)} on {v.device}" if hasattr(v, "data_ptr") else type(v).__name__
            raise ValueError(f"{fn}: want a contiguous device tensor of {n} bool or uint8 values on cuda:{self.ctx.device} for {name}, got {got}")
        return C.c_void_p(v.data_ptr() or 1)

    def mxv_frontier(self, x, x_present=None, mask=None, mask_complement=False, semiring="plus_times", transpose=False, out=None,
                     accumulate=False, out_present=None):
        """mxv with a sparse input vector and an output mask.  x, out: as for mxv (x may be None under
        plus_pair, which reads no value).  x_present: x_j takes part where its byte is nonzero (None: every x_j); mask: out_i may be
        written where (mask_i != 0) != mask_complement (None: every out_i); out_present: set to 1 where out_i is allowed and got at
        least one term, else 0.  The three are contiguous device torch.bool / torch.uint8 tensors of x's resp. out's length.  An
        allowed out_i is mxv's fold over the entries whose x_j is present -- bit for bit CPlan(A, X) with X storing the present x_j --
        and gets the start value, or stays with accumulate=True, when none is; an absent x_j is never read; a disallowed out_i is
        never written.  Lines no present x_j can reach or without an allowed output are skipped before their entries are touched.
        Ordered on the context's stream and never waits (see mxv).  Returns out."""
        if semiring not in SEMIRINGS:
            raise ValueError(f"unknown semiring {semiring!r}; one of {sorted(SEMIRINGS)}")
        nx, ny = (self.rows, self.cols) if transpose else (self.cols, self.rows)
        px = None if x is None and semiring == "plus_pair" else self._vector("mxv_frontier", "x", x, nx)
        pxp = self._bytes("mxv_frontier", "x_present", x_present, nx)
        pm = self._bytes("mxv_frontier", "mask", mask, ny)
        pyp = self._bytes("mxv_frontier", "out_present", out_present, ny)
        like = next((t for t in (x, x_present, mask, out_present) if t is not None), None)
        out, py = self._out("mxv_frontier", out, ny, like=like)
        fn = lib().pem_tiled_mxv_frontier_f32 if self.value_bytes == 4 else lib().pem_tiled_mxv_frontier
        _check(fn(self.ctx._h, self._h, SEMIRINGS[semiring], int(bool(transpose)), px, pxp, py, pm, int(bool(mask_complement)), pyp,
                  int(bool(accumulate))))
        return out

    def frontier_line_flags(self, transpose=False):
        """test hook (pem_test.h): the line flags of the context's last mxv_frontier with an x_present, one byte per 16 outputs.  Waits."""
        n = self.tile_cols if transpose else self.tile_rows
        flags = np.zeros(n, np.uint8)
        _check(lib().pem_test_frontier_line_flags(self.ctx._h, _p(flags, C.c_uint8), C.c_int64(n)))
        return flags

    def bfs(self, source, transpose=False):
        """Breadth-first search over the pattern of a square tiling: a stored entry (i, j) is an edge
        i -> j (transpose=True: j -> i).  Returns (levels, depth, reached): an int32 device torch tensor with the least number of
        edges from source to every vertex (-1: unreachable), the largest level, and the number of vertices reached.  Waits."""
        import torch
        levels = torch.empty(self.rows, dtype=torch.int32, device=torch.device("cuda", self.ctx.device))
        depth, reached = C.c_int32(), C.c_int64()
        _check(lib().pem_tiled_bfs(self.ctx._h, self._h, C.c_int64(int(source)), int(bool(transpose)), C.c_void_p(levels.data_ptr() or 1),
                                   C.byref(depth), C.byref(reached)))
        return levels, depth.value, reached.value

    def _index_out(self, fn, name, out, n, like=None):
        """(tensor, device pointer) of a contiguous torch.int32 tensor of n entries on the context's device, allocated when None"""
        import torch
        if out is None:
            dev = like.device if like is not None else torch.device("cuda", self.ctx.device)
            out = torch.empty(n, dtype=torch.int32, device=dev)
        if (not hasattr(out, "data_ptr") or not out.is_cuda or out.device.index != self.ctx.device or out.numel() != n or out.dim() != 1
                or not out.is_contiguous() or out.dtype != torch.int32):
            got = f"{out.dtype} of shape {tuple(out.shape)} on {out.device}" if hasattr(out, "data_ptr") else type(out).__name__
            raise ValueError(f"{fn}: want a contiguous device tensor of {n} int32 values on cuda:{self.ctx.device} for {name}, got {got}")
        return out, C.c_void_p(out.data_ptr() or 1)

    def mxv_arg(self, x, kind="min_plus", transpose=False, x_present=None, mask=None, mask_complement=False, out=None, out_index=None,
                out_present=None, accumulate=False):
        """Arg fold: mxv_frontier under min_plus / max_plus / max_times that also says where the minimum
        (maximum) was attained, or -- kind "min_index" / "max_index" -- only the smallest (largest) index into x of an entry that
        enters the fold.  x, x_present, mask, mask_complement, out, out_present, transpose and accumulate: as for mxv_frontier (no
        x_present and no mask: the dense case).  out_index: a contiguous device torch.int32 tensor of out's length, allocated when
        None.  Returns (out, out_index).  Under a value kind out is what mxv_frontier writes and out_index[i] the smallest index j
        whose term equals it -- ties go to the lower index, +0 == -0 -- or -1 where no term won (accumulate=True: left as it was, and
        a term wins only where it is strictly better than the old out[i] or that is NaN).  Under an index kind x may be None, no value
        is read, out is None, and with accumulate=True an old out_index[i] >= 0 takes part.  A disallowed output has nothing written.
        Ordered on the context's stream and never waits (see mxv)."""
        if kind not in ARG_KINDS:
            raise ValueError(f"unknown kind {kind!r}; one of {list(ARG_KINDS)}")
        values = kind not in INDEX_ARG_KINDS
        nx, ny = (self.rows, self.cols) if transpose else (self.cols, self.rows)
        px = self._vector("mxv_arg", "x", x, nx) if values or x is not None else None
        pxp = self._bytes("mxv_arg", "x_present", x_present, nx)
        pm = self._bytes("mxv_arg", "mask", mask, ny)
        pyp = self._bytes("mxv_arg", "out_present", out_present, ny)
        like = next((t for t in (x, x_present, mask, out_present, out_index) if t is not None), None)
        py = None
        if values:
            out, py = self._out("mxv_arg", out, ny, like=like)
        elif out is not None:
            raise ValueError(f"mxv_arg: kind {kind!r} writes no value; out must be None")
        out_index, pi = self._index_out("mxv_arg", "out_index", out_index, ny, like=like)
        fn = lib().pem_tiled_mxv_arg_f32 if self.value_bytes == 4 else lib().pem_tiled_mxv_arg
        _check(fn(self.ctx._h, self._h, ARG_KINDS.index(kind), int(bool(transpose)), px if values else None, pxp, py, pi, pm,
                  int(bool(mask_complement)), pyp, int(bool(accumulate))))
        return out, out_index

    def reduce_arg(self, op="max", dim="rows"):
        """Arg reduction: (y, idx) with y[i] the min (op="min") or max of row i's (dim="cols": column
        i's) stored values -- A.reduce(op, dim)'s values -- and idx[i], torch.int32, the smallest index inside the line where a stored
        value equals it; an empty or all-NaN line gives the identity and -1.  Ordered on the context's stream and never waits."""
        if op not in ("min", "max"):
            raise ValueError(f"unknown op {op!r}; 'min' or 'max'")
        if dim not in REDUCE_DIMS:
            raise ValueError(f"unknown dim {dim!r}; one of {sorted(REDUCE_DIMS)}")
        n = self.cols if dim == "cols" else self.rows
        out, py = self._out("reduce_arg", None, n)
        idx, pi = self._index_out("reduce_arg", "idx", None, n)
        fn = lib().pem_tiled_reduce_arg_f32 if self.value_bytes == 4 else lib().pem_tiled_reduce_arg
        _check(fn(self.ctx._h, self._h, BINOPS[op], REDUCE_DIMS[dim], py, pi))
        return out, idx

    def bfs_parents(self, source, transpose=False):
        """bfs with the breadth-first tree.  Returns (levels, parents, depth, reached): levels, depth and
        reached are bfs's; parents is an int32 device torch tensor with parents[source] = source, -1 where a vertex is unreachable,
        and otherwise the smallest-numbered vertex of the previous level with an edge to it.  Waits."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        levels = torch.empty(self.rows, dtype=torch.int32, device=dev)
        parents = torch.empty(self.rows, dtype=torch.int32, device=dev)
        depth, reached = C.c_int32(), C.c_int64()
        _check(lib().pem_tiled_bfs_parents(self.ctx._h, self._h, C.c_int64(int(source)), int(bool(transpose)),
                                           C.c_void_p(levels.data_ptr() or 1), C.c_void_p(parents.data_ptr() or 1), C.byref(depth),
                                           C.byref(reached)))
        return levels, parents, depth.value, reached.value

    def _block(self, fn, name, v, n, k=None, dtype=None):
        """(k, ld) of a 2-D row-major device torch tensor of dtype (None: this tiling's) with n rows (and k columns): stride(1) == 1
        and stride(0) >= k, so a column slice of a wider row-major tensor is accepted"""
        dtype = self.dtype if dtype is None else np.dtype(dtype)
        want = (f"a 2-D device tensor on cuda:{self.ctx.device} of {dtype.name} values, {n} x {'k' if k is None else k}, row-major "
                "(stride(1) == 1, stride(0) >= k)")
        if not hasattr(v, "data_ptr"):
            raise ValueError(f"{fn}: want {want} for {name}, got {type(v).__name__}")
        got = f"{v.dtype} of shape {tuple(v.shape)}, strides {tuple(v.stride())} on {v.device}"
        if (v.dim() != 2 or not v.is_cuda or v.device.index != self.ctx.device or str(v.dtype) != f"torch.{dtype.name}" or v.shape[0] != n
                or (k is not None and v.shape[1] != k)):
            raise ValueError(f"{fn}: want {want} for {name}, got {got}")
        kk = v.shape[1]
        if kk == 0:   # (no element: the strides say nothing)
            return 0, 1
        if (v.stride(1) != 1 and kk > 1) or (v.shape[0] > 1 and v.stride(0) < kk):
            raise ValueError(f"{fn}: want {want} for {name}, got {got}")
        return kk, v.stride(0) if v.shape[0] > 1 else kk

    def spmm(self, X, semiring="plus_times", transpose=False, out=None, accumulate=False):
        """Sparse times dense block: out = A (+).(x) X, or A^T (+).(x) X with transpose=True, under a
        semiring of SEMIRINGS.  X: a 2-D device torch tensor of the tiling's dtype, cols x k (transpose: rows x k), row-major with
        stride(1) == 1 and stride(0) >= k (a column slice of a wider tensor is fine); out: rows x k (transpose: cols x k) under the
        same rule, allocated contiguous when None.  Column c of out is bit for bit A.mxv(X[:, c], ...) with the same accumulate;
        columns past k of out's rows are never written.  X and out must not overlap.  Ordered on the context's stream and never waits
        (see mxv).  Returns out."""
        if semiring not in SEMIRINGS:
            raise ValueError(f"unknown semiring {semiring!r}; one of {sorted(SEMIRINGS)}")
        nx, ny = (self.rows, self.cols) if transpose else (self.cols, self.rows)
        k, ldx = self._block("spmm", "X", X, nx)
        if out is None:
            import torch
            out = torch.empty((ny, k), dtype=getattr(torch, self.dtype.name), device=X.device)
        _, ldy = self._block("spmm", "out", out, ny, k)
        fn = lib().pem_tiled_spmm_f32 if self.value_bytes == 4 else lib().pem_tiled_spmm
        _check(fn(self.ctx._h, self._h, SEMIRINGS[semiring], int(bool(transpose)), C.c_int64(k), C.c_void_p(X.data_ptr()), C.c_int64(ldx),
                  C.c_void_p(out.data_ptr()), C.c_int64(ldy), int(bool(accumulate))))
        return out

    def _sddmm_args(self, fn, X, Y, semiring, dtype):
        """(f32, k, X's pointer and stride, Y's pointer and stride) of an sddmm call; dtype None: X's dtype decides"""
        if semiring not in SEMIRINGS:
            raise ValueError(f"unknown semiring {semiring!r}; one of {sorted(SEMIRINGS)}")
        if dtype is None:
            name = str(getattr(X, "dtype", "")).replace("torch.", "")
            if name not in ("float32", "float64"):
                raise ValueError(f"{fn}: want a 2-D device tensor of float32 or float64 values for X, got {name or type(X).__name__}")
            dtype = np.dtype(name)
        if Y is None:
            if self.rows != self.cols:
                raise ValueError(f"{fn}: Y=None means Y = X and needs a square tiling, not {self.rows} x {self.cols}")
            Y = X
        k, ldx = self._block(fn, "X", X, self.rows, dtype=dtype)
        _, ldy = self._block(fn, "Y", Y, self.cols, k, dtype=dtype)
        return (dtype == np.float32, C.c_int64(k), C.c_void_p(X.data_ptr()), C.c_int64(ldx), C.c_void_p(Y.data_ptr()), C.c_int64(ldy))

    def sddmm(self, X, Y=None, semiring="plus_times"):
        """Sampled dense-dense product: a new tiling R with this tiling's pattern and R(i, j) = the fold
        over c of X[i, c] (x) Y[j, c] under a semiring of SEMIRINGS -- pattern(S) o (X . Y^T); this tiling's values are never read.
        X: rows x k, Y: cols x k (None: Y = X, a square tiling), 2-D device torch tensors of one dtype under spmm's rules (stride(1)
        == 1, stride(0) >= k); R's dtype is X's, whatever this tiling's.  Under plus_times every value is the chain acc = fma(X[i, c],
        Y[j, c], acc) in ascending c from 0.  Waits.  The next X, Y go into R in place with R.set_values_sddmm."""
        f32, k, px, ldx, py, ldy = self._sddmm_args("sddmm", X, Y, semiring, None)
        h = C.c_void_p()
        fn = lib().pem_tiled_sddmm_f32 if f32 else lib().pem_tiled_sddmm
        _check(fn(self.ctx._h, self._h, SEMIRINGS[semiring], k, px, ldx, py, ldy, C.byref(h)))
        return Tiled(self.ctx, h)

    def set_values_sddmm(self, X, Y=None, semiring="plus_times", accumulate=False):
        """sddmm in place: this tiling's values become the sampled product at its own pattern (X, Y of the tiling's dtype); with
        accumulate=True every fold starts from the entry's old value (lor_land: from old != 0).  Plans built on the tiling turn stale
        as after set_values.  Ordered on the context's stream and never waits (see mxv)."""
        f32, k, px, ldx, py, ldy = self._sddmm_args("set_values_sddmm", X, Y, semiring, self.dtype)
        fn = lib().pem_tiled_set_values_sddmm_f32 if f32 else lib().pem_tiled_set_values_sddmm
        _check(fn(self.ctx._h, self._h, SEMIRINGS[semiring], k, px, ldx, py, ldy, int(bool(accumulate))))

    def sampled_mxm(self, A, B, semiring="plus_times", transpose_b=False):
        """Sampled sparse product: a new tiling R with this tiling's pattern and A's dtype, R(i, j) = the
        fold, in ascending k, over the k where A(i, k) and B(k, j) (transpose_b: B(j, k)) are both stored, under a semiring of
        SEMIRINGS with step 3's arithmetic -- pattern(S) o (A . B) by dot products, at a cost that follows the pattern.  Where the
        masked plan C<S> = A . B stores an entry R holds its value bit for bit, elsewhere the semiring's start value.  This tiling's
        values are never read; S, A and B may be the same tiling.  Waits.  New operand values go into R in place with
        R.set_values_sampled_mxm."""
        if semiring not in SEMIRINGS:
            raise ValueError(f"unknown semiring {semiring!r}; one of {sorted(SEMIRINGS)}")
        h = C.c_void_p()
        _check(lib().pem_tiled_sampled_mxm(self.ctx._h, self._h, A._h, B._h, int(bool(transpose_b)), SEMIRINGS[semiring], C.byref(h)))
        return Tiled(self.ctx, h)

    def set_values_sampled_mxm(self, A, B, semiring="plus_times", transpose_b=False, accumulate=False):
        """sampled_mxm in place: this tiling's values become the sampled product at its own pattern (A, B of the tiling's dtype, neither
        of them this tiling); with accumulate=True every fold starts from the entry's old value (lor_land: from old != 0).  Plans built
        on the tiling turn stale as after set_values.  Ordered on the context's stream and never waits (see mxv)."""
        if semiring not in SEMIRINGS:
            raise ValueError(f"unknown semiring {semiring!r}; one of {sorted(SEMIRINGS)}")
        _check(lib().pem_tiled_set_values_sampled_mxm(self.ctx._h, self._h, A._h, B._h, int(bool(transpose_b)), SEMIRINGS[semiring],
                                                      int(bool(accumulate))))

    def reduce(self, op="plus", dim="rows", out=None, accumulate=False):
        """Row or column reduction: out[i] = the left fold, in ascending index, of row i's (dim="cols":
        column i's) stored values under op (one of BINOPS), from the op's identity -- or from out's old value with accumulate=True.
        out: a contiguous device torch tensor of the tiling's dtype with rows (cols) entries, allocated when None.  Ordered on the
        context's stream and never waits (a context on the torch stream torch works on needs no extra sync; see mxv).  Returns out."""
        if op not in BINOPS:
            raise ValueError(f"unknown op {op!r}; one of {sorted(BINOPS)}")
        if dim not in REDUCE_DIMS:
            raise ValueError(f"unknown dim {dim!r}; one of {sorted(REDUCE_DIMS)}")
        out, py = self._out("reduce", out, self.cols if dim == "cols" else self.rows)
        fn = lib().pem_tiled_reduce_f32 if self.value_bytes == 4 else lib().pem_tiled_reduce
        _check(fn(self.ctx._h, self._h, BINOPS[op], REDUCE_DIMS[dim], py, int(bool(accumulate))))
        return out

    def export_csr(self):
        """(rowptr int32[rows + 1], colidx int32[nnz], vals[nnz] in the tiling's dtype): the tiled matrix as canonical CSR."""
        f32 = self.value_bytes == 4
        rp, ci, v = np.zeros(self.rows + 1, np.int32), np.zeros(self.nnz, np.int32), np.zeros(self.nnz, self.dtype)
        n = C.c_int64()
        fn = lib().pem_tiled_export_csr_f32 if f32 else lib().pem_tiled_export_csr
        _check(fn(self.ctx._h, self._h, C.byref(n), _p(rp, C.c_int32), _p(ci, C.c_int32), _p(v, C.c_float if f32 else C.c_double)))
        return rp, ci, v

    def save(self, path, key=None):
        """Write the sorted tile payload to a cache file."""
        _check(lib().pem_tiled_save(self.ctx._h, self._h, os.fsencode(path), C.byref(key) if key is not None else None))

    @classmethod
    def load(cls, ctx, path, expect=None):
        """Rebuild a tiling from a cache file: upload, device-side validation, derived arrays -- no parse, no sort."""
        h = C.c_void_p()
        _check(lib().pem_tiled_load(ctx._h, os.fsencode(path), C.byref(expect) if expect is not None else None, C.byref(h)))
        return cls(ctx, h)

    def _count(self, name):
        T, nnz = self.ntiles, self.nnz
        return dict(tile_keys=T, tile_nnz_ptr=T + 1, masks=16 * T, rowptr=16 * T, rowcolidx=nnz, vals=nnz, masks_t=16 * T,
                    tile_rowptr=self.tile_rows + 1, tile_colidx=T, tile_colptr=self.tile_cols + 1, tile_rowidx=T, tile_offsets=T)[name]

    def array(self, name):
        which, dt = T_ARRAYS[name]
        if name == "vals":
            dt = self.dtype
        out = np.zeros(self._count(name), dtype=dt)
        _check(lib().pem_tiled_get_array(self.ctx._h, self._h, which, out.ctypes.data_as(C.c_void_p), C.c_int64(out.nbytes)))
        return out

    def close(self):
        if self._h:
            if self._owner is None:
                lib().pem_tiled_destroy(self.ctx._h, self._h)
            self._h, self._owner = C.c_void_p(), None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Amg:
    """pem_amg: the aggregation-multigrid hierarchy of a square tiling A with a stored diagonal, and
    one V-cycle of it as z = M r.  smooth: the Jacobi-smoothed prolongator (True) or the piecewise-constant one; symmetric, seed:
    Tiled.aggregate's, at every level; max_levels (1 .. AMG_MAX_LEVELS) and coarse_size (a level of at most that many rows is the
    coarsest) bound the hierarchy; sweeps: Jacobi sweeps before and after the coarse correction; coarse_sweeps: those on the coarsest
    level; omega: the Jacobi weight, of the smoother and of the smoothed prolongator; refreshable: keep what refresh() needs.  The
    object keeps A alive and reads its current values in refresh().  Wrong arguments raise ValueError; what the library refuses (a row
    without a stored diagonal entry, a pattern that is not symmetric under symmetric=True) raises PemError.  Waits."""

    def __init__(self, A, smooth=True, symmetric=False, seed=0, max_levels=16, coarse_size=40, sweeps=1, coarse_sweeps=4, omega=2 / 3,
                 refreshable=True):
        if not isinstance(A, Tiled):
            raise ValueError(f"Amg: A must be a tiling, not {type(A).__name__}")
        seed = _colour_seed(seed, "Amg")
        for name, v, lo, hi in (("max_levels", max_levels, 1, AMG_MAX_LEVELS), ("coarse_size", coarse_size, 1, 2 ** 63 - 1),
                                ("sweeps", sweeps, 1, 2 ** 31 - 1), ("coarse_sweeps", coarse_sweeps, 1, 2 ** 31 - 1)):
            if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not lo <= int(v) <= hi:
                raise ValueError(f"Amg: {name} must be an integer in [{lo}, {hi}], not {v!r}")
        if isinstance(omega, bool) or not isinstance(omega, numbers.Real) or not (float(omega) > 0 and np.isfinite(float(omega))):
            raise ValueError(f"Amg: omega must be a positive finite number, not {omega!r}")
        self.A, self.ctx = A, A.ctx
        self.opts = dict(smooth=bool(smooth), symmetric=bool(symmetric), seed=seed, max_levels=int(max_levels), coarse_size=int(coarse_size),
                         sweeps=int(sweeps), coarse_sweeps=int(coarse_sweeps), omega=float(omega), refreshable=bool(refreshable))
        o = AmgOpts(int(bool(smooth)), int(bool(symmetric)), seed, int(max_levels), int(coarse_size), int(sweeps), int(coarse_sweeps),
                    float(omega), int(bool(refreshable)))
        self._h = C.c_void_p()
        _check(lib().pem_amg_create(self.ctx._h, A._h, C.byref(o), C.byref(self._h)))

    @property
    def info(self):
        """dict: levels; rows, nnz (of every A_l), p_nnz (of every P_l, 0 at the coarsest), aggregate_rounds: lists of `levels`
        entries; launches (of one apply, the mxv launches included); bytes (device bytes beyond A itself);
        operator_complexity = sum(nnz) / nnz[0]"""
        m = AmgInfo()
        _check(lib().pem_amg_get_info(self._h, C.byref(m)))
        n = int(m.levels)
        out = dict(levels=n, rows=list(m.rows[:n]), nnz=list(m.nnz[:n]), p_nnz=list(m.p_nnz[:n]),
                   aggregate_rounds=list(m.aggregate_rounds[:n]), launches=int(m.launches), bytes=int(m.bytes))
        out["operator_complexity"] = sum(out["nnz"]) / out["nnz"][0] if out["nnz"][0] else 1.0
        return out

    @property
    def levels(self):
        return self.info["levels"]

    def level(self, l):
        """(A_l, P_l, R_l): non-owning Tiled views, valid while this object is open (each keeps it alive); P_l and R_l = P_l^T are
        None at the coarsest level.  close() on a view does not destroy the tiling."""
        if isinstance(l, bool) or not isinstance(l, numbers.Integral):
            raise ValueError(f"Amg.level: the level must be an integer, not {l!r}")
        h = [C.c_void_p(), C.c_void_p(), C.c_void_p()]
        _check(lib().pem_amg_get_level(self._h, int(l), *(C.byref(x) for x in h)))
        return tuple(Tiled(self.ctx, x, owner=self) if x.value else None for x in h)

    def apply(self, r, out=None):
        """out = one V-cycle on A z = r from z = 0.  r: a contiguous device torch tensor of A's dtype with A.rows entries; out: one
        like it, not overlapping r, allocated when None.  Ordered on the context's stream, never waits (see Tiled.mxv).  Returns out."""
        A = self.A
        pr = A._vector("Amg.apply", "r", r, A.rows)
        out, pz = A._out("Amg.apply", out, A.rows, like=r)
        fn = lib().pem_amg_apply_f32 if A.value_bytes == 4 else lib().pem_amg_apply
        _check(fn(self.ctx._h, self._h, pr, pz))
        return out

    def refresh(self):
        """After new values on A (same pattern): every level's values again on the patterns and aggregates the setup found -- what
        a fresh Amg on the new values holds, array for array.  Ordered on the context's stream, reads nothing back; allocates nothing
        from the second call on.  PemError (PEM_E_STATE) with refreshable=False."""
        _check(lib().pem_amg_refresh(self.ctx._h, self._h))

    def close(self):
        if self._h:
            lib().pem_amg_destroy(self.ctx._h, self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Krylov:
    """pem_krylov: preconditioned CG or BiCGStab on a square tiling A, the whole loop on the context's
    stream.  method: one of KRYLOV_METHODS.  precond: None or "none"; "diag" (every solve then takes minv); a tiling F, an LU
    factor such as A.ilu0(), applied by two trsv; or an Amg made on A, applied as one V-cycle (Krylov.precond then reads "amg").  The host reads a 128-byte state block back every check_every iterations; x, iters,
    status and the history do not depend on check_every.  Stops at rr <= max(rtol^2 * bb, atol^2), after max_iters iterations, on
    a breakdown or on a residual that is not finite.  The object keeps A, F and the Amg alive and reads their current values in every
    solve.
    Wrong arguments raise ValueError; what the library refuses raises PemError."""

    def __init__(self, A, method="cg", precond=None, max_iters=1000, check_every=8, rtol=1e-8, atol=0.0):
        if method not in KRYLOV_METHODS:
            raise ValueError(f"Krylov: unknown method {method!r}; one of {KRYLOV_METHODS}")
        F = M = None
        if precond is None or (isinstance(precond, str) and precond == "none"):
            pc = 0
        elif isinstance(precond, str) and precond == "diag":
            pc = 1
        elif isinstance(precond, Tiled):
            pc, F = 2, precond
        elif isinstance(precond, Amg):
            pc, M = PRECOND_AMG, precond
        else:
            raise ValueError(f"Krylov: precond must be None, 'none', 'diag', a tiling (an LU factor) or an Amg, not {precond!r}")
        for name, v in (("max_iters", max_iters), ("check_every", check_every)):
            if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not -2 ** 63 <= int(v) < 2 ** 63:
                raise ValueError(f"Krylov: {name} must be an integer, not {v!r}")
        for name, v in (("rtol", rtol), ("atol", atol)):
            if isinstance(v, bool) or not isinstance(v, numbers.Real):
                raise ValueError(f"Krylov: {name} must be a real number, not {v!r}")
        self.A, self.F, self.M, self.ctx = A, F, M, A.ctx
        self.method, self.precond = method, "amg" if M is not None else KRYLOV_PRECONDS[pc]
        self.max_iters, self.check_every = int(max_iters), int(check_every)
        opts = KrylovOpts(KRYLOV_METHODS.index(method), pc, int(max_iters), int(check_every), float(rtol), float(atol))
        self._h = C.c_void_p()
        if M is not None:
            _check(lib().pem_krylov_create_amg(self.ctx._h, A._h, C.byref(opts), M._h, C.byref(self._h)))
        else:
            _check(lib().pem_krylov_create(self.ctx._h, A._h, C.byref(opts), F._h if F is not None else None, C.byref(self._h)))

    def solve(self, b, x=None, minv=None, history=False):
        """(x, info).  b: a contiguous device torch tensor of A's dtype with A.rows entries; x: the guess, overwritten with the
        solution and returned (None: a zero guess); minv: the inverse diagonal, required under "diag" and refused otherwise; history:
        True records the squared residual norm of every iteration.  info: iters, status (one of KRYLOV_STATUS), status_code, bb, rr,
        threshold, rnorm = sqrt(rr), readbacks, launches and, with history=True, history -- a float64 device tensor of iters + 1
        entries.  A status other than "converged" is no error.  Waits for its read-backs only; torch reads x with no extra sync on a
        context created on torch's stream."""
        import torch
        A = self.A
        pb = A._vector("Krylov.solve", "b", b, A.rows)
        if x is None:
            x = torch.zeros(A.rows, dtype=b.dtype, device=b.device)
            if A.rows:
                torch.cuda.current_stream(b.device).synchronize()   # (torch's fill; x is read on the context's stream)
        px = A._vector("Krylov.solve", "x", x, A.rows)
        if (minv is not None) != (self.precond == "diag"):
            raise ValueError("Krylov.solve: minv is required with precond='diag' and refused without it")
        pm = A._vector("Krylov.solve", "minv", minv, A.rows) if minv is not None else None
        hist = None
        if hasattr(history, "data_ptr"):   # the caller's buffer: max_iters + 1 float64 on the device; entries past iters stay as they are
            hist = history
            if not hist.is_cuda or hist.dtype != torch.float64 or hist.numel() != self.max_iters + 1 or not hist.is_contiguous():
                raise ValueError(f"Krylov.solve: want a contiguous device tensor of {self.max_iters + 1} float64 values for history")
        elif history:
            hist = torch.empty(self.max_iters + 1, dtype=torch.float64, device=b.device)
        res = KrylovResult()
        fn = lib().pem_krylov_solve_f32 if A.value_bytes == 4 else lib().pem_krylov_solve
        _check(fn(self.ctx._h, self._h, pb, px, pm, C.c_void_p(hist.data_ptr()) if hist is not None else None, C.byref(res)))
        info = dict(iters=int(res.iters), status=KRYLOV_STATUS[res.status], status_code=int(res.status), bb=res.bb, rr=res.rr,
                    threshold=res.threshold, rnorm=float(np.sqrt(res.rr)) if res.rr >= 0 else float("nan"), readbacks=int(res.readbacks),
                    launches=int(res.launches))
        if hist is not None:
            info["history"] = hist[:info["iters"] + 1]
        return x, info

    def close(self):
        if self._h:
            lib().pem_krylov_destroy(self.ctx._h, self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def krylov_dot(ctx, u, v):
    """test hook (pem_test.h): the solvers' dot product of two contiguous device tensors of one dtype (float32 / float64), as a float"""
    if u.dtype != v.dtype or u.numel() != v.numel() or str(u.dtype) not in ("torch.float32", "torch.float64"):
        raise ValueError("krylov_dot: want two device tensors of one length and dtype (float32 or float64)")
    out = C.c_double()
    _check(lib().pem_test_krylov_dot(ctx._h, u.numel(), u.element_size(), C.c_void_p(u.data_ptr() or 1), C.c_void_p(v.data_ptr() or 1),
                                     C.byref(out)))
    return out.value


def flop_count(ctx, A, B):
    f = C.c_uint64()
    _check(lib().pem_flop_count(ctx._h, A._h, B._h, C.byref(f)))
    return f.value


def split_tile_rows(ctx, A, B, nparts):
    b = np.zeros(nparts + 1, dtype=np.int32)
    _check(lib().pem_split_tile_rows(ctx._h, A._h, B._h, int(nparts), _p(b, C.c_int32)))
    return b


def tile_row_weights(ctx, A, B):
    """the per-tile-row weights pem_split_tile_rows balances (float64, one per tile row of A)"""
    w = np.zeros(A.tile_rows, dtype=np.float64)
    _check(lib().pem_tile_row_weights(ctx._h, A._h, B._h, _p(w, C.c_double)))
    return w


def triangle_count(A):
    """The triangles of the graph whose adjacency pattern A stores (a symmetric pattern; values and the diagonal are not read):
    with L = A's strict lower triangle, the sum of L o (L . L^T) under plus_pair -- every triangle i > j > k counted once, at its
    edge (i, j).  Three device calls (select, sampled_mxm, reduce); returns an int."""
    L = A.select("tril", -1)
    R = L.sampled_mxm(L, L, "plus_pair", transpose_b=True)
    per_row = R.reduce("plus", "rows")
    A.ctx.synchronize()
    return int(round(float(per_row.double().sum().item())))


def _colour_seed(seed, fn="colour"):
    """Tiled.colour's (mis', aggregate's) seed: an integer in [0, 2^32)"""
    if isinstance(seed, bool) or not isinstance(seed, numbers.Integral) or not 0 <= int(seed) < 2 ** 32:
        raise ValueError(f"{fn}: seed must be an integer in [0, 2^32), not {seed!r}")
    return int(seed)


def _colour_priority(priority, n, fn="colour"):
    """Tiled.colour's (mis', aggregate's) host priorities -> a contiguous uint32 array of n entries"""
    a = np.asarray(priority)
    if a.ndim != 1 or a.size != n:
        raise ValueError(f"{fn}: priority must hold {n} entries, one per vertex, not shape {a.shape}")
    if a.size and a.dtype.kind not in "iu":
        raise ValueError(f"{fn}: priority must hold integers, not {a.dtype}")
    if a.size and (int(a.min()) < 0 or int(a.max()) >= 2 ** 32):
        raise ValueError(f"{fn}: priority holds a value outside [0, 2^32)")
    return np.ascontiguousarray(a, dtype=np.uint32)


def prolongator(ctx, agg, naggregates, values=None, dtype=np.float64):
    """The piecewise-constant prolongator of an aggregation: the n x naggregates tiling P with one entry
    per row, at (v, agg[v]), of value 1 -- or values[v], a near-null-space vector.  agg: Tiled.aggregate's contiguous 1-d int32
    tensor on the context's device; an entry outside [0, naggregates) (the -1 a false symmetric=True promise leaves) is refused.
    values: a contiguous device tensor of n values of `dtype`, or None.  Made by Tiled.from_coo_device: nothing leaves the device
    but the one flag of the range check.  Waits."""
    if isinstance(naggregates, bool) or not isinstance(naggregates, numbers.Integral) or not 0 <= int(naggregates) < 2 ** 31:
        raise ValueError(f"prolongator: naggregates must be an integer in [0, 2^31), not {naggregates!r}")
    if (not hasattr(agg, "data_ptr") or not agg.is_cuda or agg.device.index != ctx.device or agg.dim() != 1 or not agg.is_contiguous()
            or str(agg.dtype) != "torch.int32"):
        got = f"{agg.dtype} of shape {tuple(agg.shape)} on {agg.device}" if hasattr(agg, "data_ptr") else type(agg).__name__
        raise ValueError(f"prolongator: want a contiguous 1-d int32 tensor on cuda:{ctx.device} for agg, got {got}")
    import torch
    n = agg.numel()
    tdtype = torch.float32 if np.dtype(dtype) == np.float32 else torch.float64
    if values is None:
        values = torch.ones(n, dtype=tdtype, device=agg.device)
    elif (not hasattr(values, "data_ptr") or not values.is_cuda or values.device != agg.device or values.dim() != 1 or values.numel() != n
            or not values.is_contiguous() or values.dtype != tdtype):
        got = f"{values.dtype} of shape {tuple(values.shape)} on {values.device}" if hasattr(values, "data_ptr") else type(values).__name__
        raise ValueError(f"prolongator: want a contiguous device tensor of {n} {tdtype} values on {agg.device} for values, got {got}")
    if n and bool(((agg < 0) | (agg >= int(naggregates))).any()):
        raise ValueError(f"prolongator: agg holds an entry outside [0, {int(naggregates)}): a vertex without an aggregate has no row of P")
    rows = torch.arange(n, dtype=torch.int32, device=agg.device)
    torch.cuda.current_stream(agg.device).synchronize()   # (the triplets are read on the context's stream)
    P = Tiled.from_coo_device(ctx, n, int(naggregates), n, rows.data_ptr() or 1, agg.data_ptr() or 1, values.data_ptr() or 1, dtype=dtype)
    ctx.synchronize()   # (rows and a default values are freed on return)
    return P


def colour_order(ctx, colours, ncolours):
    """The stable counting sort by colour: (perm, offsets), int32 device torch tensors -- perm the
    vertices colour by colour, ascending inside a colour (np.argsort(colours, kind="stable")), offsets (ncolours + 1 entries) with
    colour c = perm[offsets[c]:offsets[c + 1]].  colours: a contiguous 1-d int32 torch tensor on the context's device with values
    in [0, ncolours) (any such key sorts: Tiled.components' ids with its ncomponents give the component order) -- a value outside
    raises PemError; ncolours: an integer >= 0, at least 1 where colours has entries.  perm goes
    straight into Tiled.extract as both lists.  Waits."""
    if isinstance(ncolours, bool) or not isinstance(ncolours, numbers.Integral) or not 0 <= int(ncolours) < 2 ** 31:
        raise ValueError(f"colour_order: ncolours must be an integer in [0, 2^31), not {ncolours!r}")
    if (not hasattr(colours, "data_ptr") or not colours.is_cuda or colours.device.index != ctx.device or colours.dim() != 1
            or not colours.is_contiguous() or str(colours.dtype) != "torch.int32"):
        got = f"{colours.dtype} of shape {tuple(colours.shape)} on {colours.device}" if hasattr(colours, "data_ptr") else type(colours).__name__
        raise ValueError(f"colour_order: want a contiguous 1-d int32 tensor on cuda:{ctx.device} for colours, got {got}")
    n = colours.numel()
    if n and not ncolours:
        raise ValueError(f"colour_order: ncolours = 0 for {n} vertices")
    import torch
    perm = torch.empty(n, dtype=torch.int32, device=colours.device)
    offsets = torch.empty(int(ncolours) + 1, dtype=torch.int32, device=colours.device)
    _check(lib().pem_colour_order(ctx._h, C.c_int64(n), C.c_void_p(colours.data_ptr() or 1), C.c_int32(int(ncolours)),
                                  C.c_void_p(perm.data_ptr() or 1), C.c_void_p(offsets.data_ptr())))
    return perm, offsets


class CPlan:
    """pem_cplan: C = A*B over tile rows [tile_row_begin, tile_row_end) of A (steps 1-3).

    mask: a Tiled M of C's shape (A.rows x B.cols): the plan computes C<M>, only the entries of A*B at M's stored positions --
    with complement=True only those where M stores nothing (pem_cplan_create_masked).  The plan keeps a reference to M.
    semiring: a name of SEMIRINGS -- how step 3 reduces the products of each entry (pem_cplan_set_semiring)."""

    def __init__(self, ctx, A, B, tile_row_begin=0, tile_row_end=-1, mask=None, complement=False, semiring="plus_times"):
        if semiring not in SEMIRINGS:
            raise ValueError(f"unknown semiring {semiring!r}; one of {sorted(SEMIRINGS)}")
        self.ctx, self.A, self.B, self.mask = ctx, A, B, mask
        self._h = C.c_void_p()
        if mask is None:
            _check(lib().pem_cplan_create(ctx._h, A._h, B._h, int(tile_row_begin), int(tile_row_end), C.byref(self._h)))
        else:
            flags = MASK_COMPLEMENT if complement else MASK_STRUCTURE
            _check(lib().pem_cplan_create_masked(ctx._h, A._h, B._h, mask._h, flags, int(tile_row_begin), int(tile_row_end),
                                                 C.byref(self._h)))
        if semiring != "plus_times":
            self.set_semiring(semiring)

    def set_semiring(self, name):
        """pem_cplan_set_semiring: C's values are stale (exports raise PEM_E_STATE) until step3() or spgemm() runs again"""
        if name not in SEMIRINGS:
            raise ValueError(f"unknown semiring {name!r}; one of {sorted(SEMIRINGS)}")
        _check(lib().pem_cplan_set_semiring(self._h, SEMIRINGS[name]))

    @property
    def semiring(self):
        v = C.c_int()
        _check(lib().pem_cplan_get_semiring(self._h, C.byref(v)))
        return {v_: k for k, v_ in SEMIRINGS.items()}[v.value]

    def set_option(self, name, value):
        """pem_cplan_set_option: kernel variants / test hooks (OPTIONS); the next pass is a full one"""
        _check(lib().pem_cplan_set_option(self._h, OPTIONS[name], C.c_int64(int(value))))

    def get_option(self, name):
        v = C.c_int64()
        _check(lib().pem_cplan_get_option(self._h, OPTIONS[name], C.byref(v)))
        return v.value

    def step1(self):
        _check(lib().pem_spgemm_step1(self.ctx._h, self._h))

    def step2(self):
        _check(lib().pem_spgemm_step2(self.ctx._h, self._h))

    def step3(self):
        _check(lib().pem_spgemm_step3(self.ctx._h, self._h))

    def spgemm(self):
        _check(lib().pem_spgemm(self.ctx._h, self._h))

    def info(self):
        i = CPlanInfo()
        _check(lib().pem_cplan_get_info(self._h, C.byref(i)))
        return {k: getattr(i, k) for k, _ in CPlanInfo._fields_}

    def array(self, name):
        which, dt = C_ARRAYS[name] if name in C_ARRAYS else C_TEST_ARRAYS[name]
        i = self.info()
        TC, P, NZ, mt = i["ntiles_c"], i["npairs"], i["nnz_c"], i["tile_row_end"] - i["tile_row_begin"]
        cnt = dict(c_tile_rowptr=mt + 1, c_tile_rowidx=TC, c_tile_colidx=TC, pairs_offset=TC + 1, pairs_a=P, pairs_b=P, c_mask=8 * TC,
                   c_tile_nnz_ptr=TC + 1, c_rowptr=16 * TC, c_rowcolidx=NZ, c_vals=NZ, c_mtile=TC)[name]
        if name == "c_vals":
            dt = self.A.dtype
        out = np.zeros(cnt, dtype=dt)
        _check(lib().pem_cplan_get_array(self.ctx._h, self._h, which, out.ctypes.data_as(C.c_void_p), C.c_int64(out.nbytes)))
        return out

    def export_csr(self):
        i = self.info()
        nrows, nz = i["row_end"] - i["row_begin"], i["nnz_c"]
        f32 = self.A.value_bytes == 4
        rp, ci, v = np.zeros(nrows + 1, np.int32), np.zeros(nz, np.int32), np.zeros(nz, self.A.dtype)
        n = C.c_int64()
        fn = lib().pem_c_export_csr_f32 if f32 else lib().pem_c_export_csr
        _check(fn(self.ctx._h, self._h, C.byref(n), _p(rp, C.c_int32), _p(ci, C.c_int32), _p(v, C.c_float if f32 else C.c_double)))
        return rp, ci, v

    def export_csr_device(self, d_rowptr, d_colidx, d_vals):
        """d_vals points at values of the plan's type (float64, or float32 for fp32 tilings)."""
        fn = lib().pem_c_export_csr_device_f32 if self.A.value_bytes == 4 else lib().pem_c_export_csr_device
        _check(fn(self.ctx._h, self._h, C.c_void_p(d_rowptr), C.c_void_p(d_colidx), C.c_void_p(d_vals)))

    def export_coo(self):
        nz = self.info()["nnz_c"]
        f32 = self.A.value_bytes == 4
        r, c, v = np.zeros(nz, np.int32), np.zeros(nz, np.int32), np.zeros(nz, self.A.dtype)
        n = C.c_int64()
        fn = lib().pem_c_export_coo_f32 if f32 else lib().pem_c_export_coo
        _check(fn(self.ctx._h, self._h, C.byref(n), _p(r, C.c_int32), _p(c, C.c_int32), _p(v, C.c_float if f32 else C.c_double)))
        return r, c, v

    def close(self):
        if self._h:
            lib().pem_cplan_destroy(self.ctx._h, self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
