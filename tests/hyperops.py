"""What the large-dimension GPU tests share (test_gpu_bigdims.py part 2 and test_gpu_bigdims_ops.py): the hypersparse operands, built
once per dtype with the host data their references need, the comparison rules of the operations' own test files, and the kernel
profile of a block of calls.  A plain module: no test lives here."""
import numpy as np
import torch

import compactref
from compactref import T_NAMES
from matgen import hypersparse, hypersparse_diag

SCAN_CHAINED_MAX = 262_144       # SCAN_MID_ITEMS * SCAN_MID_BLOCKS: longer arrays take the three-launch scan
SORT_BLOCK_KEYS = 4096           # keys per block of the radix sort; its histogram scan is 256 words per block
TILE_LINES_MAX = 1 << 26         # from here on the `tile lines * 64` launches wrap and would hang, not fail
DTYPES = (np.float64, np.float32)
IDS = ("f64", "f32")
INFO = ("rows", "cols", "nnz", "tile_rows", "tile_cols", "ntiles", "value_bytes")
MINMAX = ("min_plus", "max_plus", "max_times", "min", "max")


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32) if a.dtype.kind == "f" else a


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


class _Profiled:
    """kernel names of the launches inside the block -> .names (and .stats: name -> calls, total_ms)"""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.ctx.set_kernel_profiling(True)
        self.ctx.reset_kernel_stats()
        return self

    def __exit__(self, *exc):
        self.stats = self.ctx.kernel_stats()
        self.names = set(self.stats)
        self.ctx.set_kernel_profiling(False)

    def calls(self, name):
        return self.stats[name]["calls"] if name in self.stats else 0


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _same_vec(got, want, kind="plus_times"):
    """the rule of test_gpu_mxv.py: bit for bit, NaN payloads not compared, zero signs free under min / max"""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    ok = (got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want))
    if kind in MINMAX:
        ok |= (got == 0) & (want == 0)
    return bool(np.all(ok))


def _assert_same_tiling(got, want, label, past=True):
    """the rule of the derived operations' own tests: every info field and all twelve arrays equal those of the tiling from_coo
    builds from the reference's entries, values bit for bit (from_coo itself is held to the lifted oracle at this size below)"""
    for k in INFO:
        assert getattr(got, k) == getattr(want, k), f"{label}: {k} {getattr(got, k)} != {getattr(want, k)}"
    for name in T_NAMES:
        assert _same(got.array(name), want.array(name)), f"{label}: array {name} differs"
    if past:
        assert min(got.tile_rows, got.tile_cols, got.ntiles) > SCAN_CHAINED_MAX, f"{label}: the result is not past the chained scan"


def _canonical(I, J, V, cols):
    o = np.argsort(np.asarray(I, np.int64) * cols + np.asarray(J), kind="stable")
    return np.asarray(I, np.int32)[o], np.asarray(J, np.int32)[o], np.asarray(V)[o]


def _bounded(T):
    """a tiling of these tests stays below the tile-line count at which a launch would wrap"""
    assert max(T.tile_rows, T.tile_cols) < TILE_LINES_MAX, f"{T.tile_rows} x {T.tile_cols} tile lines: past what DESIGN.md section 7 allows"
    return T


def bits_for(count):
    """pem_internal.h bits_for: the bits of the values in [0, count), at least 1"""
    return max(1, int(count - 1).bit_length())


def sort_passes(key_bits, first_bit=0):
    """launches of rs_scatter_kernel in one radix sort of more than one key: a pass per 8 bits"""
    return -(-(key_bits - first_bit) // 8)


def derive_passes(T):
    """the sort every new tiling ends with: its tiles by tile column, on the tile-column digits alone"""
    return sort_passes(bits_for(T.tile_cols)) if T.ntiles > 1 else 0


class _Hyper:
    source = staticmethod(hypersparse)

    def __init__(self, pkg, ctx, dtype):
        self.n, self.I, self.J, V, self.S = self.source()
        n = self.n
        self.dtype = np.dtype(dtype)
        self.V = V.astype(dtype)
        self.A = _bounded(pkg.Tiled.from_coo(ctx, n, n, self.I, self.J, self.V, dtype=dtype))
        assert min(self.A.tile_rows, self.A.tile_cols, self.A.ntiles, self.A.nnz) > SCAN_CHAINED_MAX
        self.coo = _canonical(self.I, self.J, self.V, n)                      # sorted by (row, column)
        self.map = compactref.IndexMap(np.concatenate([self.I, self.J]), n)   # the vector references run on the used lines
        self.ccsr = self.map.csr(self.I, self.J, self.V)
        self._c = {}

    def product(self, oracle, V=None):
        """lifted COO of A*A by the serial CSR oracle (cached for the tiling's own values)"""
        f32 = self.dtype == np.float32
        if V is not None:
            return compactref.product_coo(oracle, self.n, (self.I, self.J, V), (self.I, self.J, V), f32=f32)
        if "c" not in self._c:
            self._c["c"] = compactref.product_coo(oracle, self.n, (self.I, self.J, self.V), (self.I, self.J, self.V), f32=f32)
            if f32:
                self._c["c"] = (*self._c["c"][:2], self._c["c"][2].astype(np.float32))
        return self._c["c"]

    def csr(self):
        """the full-length CSR (int64 rowptr of n + 1) for the references that want one"""
        if "csr" not in self._c:
            rp = np.zeros(self.n + 1, np.int64)
            np.cumsum(np.bincount(self.I, minlength=self.n), out=rp[1:])
            self._c["csr"] = (rp, self.coo[1].astype(np.int64), self.coo[2])
        return self._c["csr"]

    def offmap(self):
        """the IndexMap over the indices with an off-diagonal entry: where the graph routines and the solves have work"""
        if "off" not in self._c:
            self._c["off"] = compactref.offdiag_map(self.n, self.I, self.J)
        return self._c["off"]

    def cached(self, key, make):
        """a host reference computed once per operand and left unchanged"""
        if key not in self._c:
            self._c[key] = make()
        return self._c[key]


class _HyperDiag(_Hyper):
    source = staticmethod(hypersparse_diag)


_HYPER = {}


def _hyper(pkg, ctx, dtype, diag=False):
    """the operand of a dtype on a context, built once (diag: hypersparse_diag's); another module's context lets the earlier ones go"""
    key = (id(ctx), np.dtype(dtype).name, bool(diag))
    for other in [k for k in _HYPER if k[0] != id(ctx)]:
        del _HYPER[other]
    if key not in _HYPER:
        _HYPER[key] = (_HyperDiag if diag else _Hyper)(pkg, ctx, dtype)
    return _HYPER[key]
