"""Host model of one context's handles for the operation-sequence test (tests/seqgen.py writes the programs, tests/seqrun.py runs
them on the GPU next to this model; DESIGN.md, "Sequence test").

Plain Python / numpy, no GPU import.  The model holds, per live handle, what include/pem_spgemm.h lets a caller observe:

  MTiled  rows, cols, dtype, the canonical CSR (rowptr, colidx, vals), a value version, and the provenance pem_internal.h's
          Derivation keeps (none / plan + transpose / ewise operands + op + pattern + alpha + beta / select source + op + thunk;
          of the second operation set: apply source + op + thunk / scale source + op / transpose source / extract source + lists /
          assign C + A + lists + accum / kron operands + op / concat cells + grid + sizes / build triplet source + dup op + nnz_in /
          ilu0 source), and which lazily built structures it holds (the refresh maps, the two trsv schedules)
  MPlan   its operands, mask + complement, tile-row range, semiring, options, state 0-3, C as CSR, and the operand versions and
          semiring under which step 3 last ran: "C is current" is computed from those, never assumed
  MKrylov the ids of A and of its factor or hierarchy (handles, not copies: a solve reads their current values) and create's options
  MAmg    the id of A, create's options and amgref's levels as of the last create or refresh -- a refresh is a rebuild from A's
          current values, the header's "array for array"; level 0's matrix is A itself, read as it is now

Model.apply(record) executes one record of a program.  It first evaluates the precondition the header documents and returns either
the result or the documented status (PEM_E_STATE, PEM_E_INVALID); only refusals the header spells out are modelled.  It adds no
arithmetic: every value comes from the reference the feature's own GPU test uses (oracle.csr_spgemm, semiringref, maskref,
ewiseref, selectref, mxvref, spmmref, sddmmref; applyref, extractref, assignref, kronref, concatref, buildref, topkref,
sampledref, frontierref, argref, trsvref, ilu0ref; of the third set colourref, ccref, aggref, krylovref, amgref, with numpy's stable
argsort for the colour order); what is here is the reshaping between CSR and COO those references ask for.

`mutations` switches on one of nine deliberate mistakes of the MODEL (negative controls of tests/test_gpu_seq.py; the library
is never touched): "no_bump" (a refresh leaves the value version alone), "stale_vals_t" (in-place writers leave the values the
audit's vals_t readers use as they were), "no_option_reset" (set_option leaves the plan's state alone), "concat_stale_block" (a
concat's refresh takes the blocks' values as of its first refresh: a pointer table that is not rewritten), "ilu0_stale_source"
(set_values_from_ilu0 factors the source's values as of the build), "trsv_stale_values" (a solve takes the values the tiling had
when that triangle's schedule was built), "amg_stale_weights" (a refresh leaves the weights of levels >= 1 as they were),
"krylov_stale_factor" (a solve takes the factor's values as of create), "colour_ties_high" (a colouring's ties go to the higher index).
"""
import numpy as np

import aggref
import amgref
import applyref
import argref
import assignref
import buildref
import ccref
import colourref
import concatref
import ewiseref
import extractref
import frontierref
import ilu0ref
import kronref
import krylovref
import maskref
import mxvref
import sampledref
import sddmmref
import selectref
import semiringref
import spmmref
import topkref
import trsvref
from matgen import cases

PEM_OK, PEM_E_INVALID, PEM_E_STATE = 0, -1, -6
MINMAX = ("min_plus", "max_plus", "max_times")
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3.0e-310, 1.0e-40, 0.5, -0.5, 2.0])   # test_gpu_sddmm.py's mix
MUTATIONS = ("no_bump", "stale_vals_t", "no_option_reset", "concat_stale_block", "ilu0_stale_source", "trsv_stale_values",
             "amg_stale_weights", "krylov_stale_factor", "colour_ties_high")
# the third operation set (seqgen.py): the graph routines, and the solve of a pem_krylov by status
GRAPH_KINDS = ("colour", "colour_order", "components", "mis", "aggregate")
AMG_OMEGA = 2 / 3                        # tests/amgcases.py's, with seed 0 and max_levels 16
# the derivation kinds of the second operation set (seqgen.py): each has a set_values_from_<kind>
KINDS2 = ("apply", "scale", "transpose", "extract", "assign", "kron", "concat", "ilu0")

# pem_cplan_set_option: the options the generator draws from, their defaults (pem_internal.h), whether the value is kept as an
# integer (else as value != 0), and the step the plan falls back to (spgemm.hip: "the last step the option does not touch")
OPTION_DEFAULT = dict(prune=1, wide=1, s3_band=1, s3_decode=1, s3_epw=0, s3_idx64=0, s3_mark=1, s3_xcd=1, s2_transposed=2,
                      s1_segments=0, s1_xl_global=0, s1_force_key64=0)
OPTION_INT = ("s3_epw", "s2_transposed")
OPTION_KEEP = dict(prune=0, s1_force_key64=0, s1_xl_global=0, s1_segments=0, wide=1, s3_decode=1, s2_transposed=1, s3_band=2,
                   s3_epw=2, s3_idx64=2, s3_mark=2, s3_xcd=2)

_CASES = None
_ORACLE = None


def oracle():
    global _ORACLE
    if _ORACLE is None:
        import __graft_entry__ as g
        _ORACLE = g.load_oracle()
    return _ORACLE


def case(name):
    global _CASES
    if _CASES is None:
        _CASES = cases()
    return _CASES[name]


def rand_matrix(seed, rows, cols, nnz, clustered):
    """test_gpu_sweep.py's _rand under a seed of its own: (I, J, V) in shuffled file order"""
    rng = np.random.default_rng(seed)
    nnz = min(nnz, rows * cols)
    if clustered:
        keys = set()
        for _ in range(max(1, nnz // 200)):
            r0, c0 = int(rng.integers(0, rows)), int(rng.integers(0, cols))
            rr = np.clip(r0 + rng.integers(-8, 9, 200), 0, rows - 1)
            cc = np.clip(c0 + rng.integers(-8, 9, 200), 0, cols - 1)
            keys.update((rr.astype(np.int64) * cols + cc).tolist())
        keys = np.sort(np.fromiter(keys, dtype=np.int64))[:nnz]
    else:
        keys = rng.choice(rows * cols, nnz, replace=False)
    v = rng.uniform(-1, 1, len(keys))
    v[v == 0] = 0.5
    p = rng.permutation(len(keys))
    return (keys[p] // cols).astype(np.int32), (keys[p] % cols).astype(np.int32), v[p]


_SQUARE = {}
_SYSTEMS = None


def square_case(kind, name, side=0):
    """a square matrix that stores its diagonal, from the triangular-solve tests' list (side 0: the lower case, 1: the upper) or
    the ILU(0) tests'"""
    if kind not in _SQUARE:
        import ilu0cases
        import trsvcases
        _SQUARE[kind] = (trsvcases if kind == "trsv" else ilu0cases).cases()
    c = _SQUARE[kind][name]
    n, I, J, V = c[side] if kind == "trsv" else c
    return n, n, np.asarray(I, np.int32), np.asarray(J, np.int32), np.asarray(V, np.float64)


def rand_square(seed, n, nnz):
    """rand_matrix's entries off the diagonal plus the whole diagonal, with trsvcases' dominant diagonal values"""
    I, J, V = rand_matrix(seed, n, n, nnz, False)
    off = I != J
    I, J, V = I[off], J[off], V[off]
    rng = np.random.default_rng(seed + 1)
    s = np.zeros(n)
    np.add.at(s, I, np.abs(V))
    d = (s + 1.0 + rng.random(n)) * rng.choice([-1.0, 1.0], n)
    k = np.arange(n, dtype=np.int32)
    return np.concatenate([I, k]), np.concatenate([J, k]), np.concatenate([V, d])


def matrix(src):
    """(rows, cols, I, J, V) of a record's matrix source: {"case": name}, {"rand": [seed, rows, cols, nnz, clustered]} or, square
    with the diagonal stored, {"trsv": [name, side]}, {"ilu0": name}, {"randdiag": [seed, n, nnz]}"""
    if "case" in src:
        rows, cols, I, J, V, _ = case(src["case"])
        return rows, cols, I, J, V
    if "trsv" in src:
        return square_case("trsv", src["trsv"][0], src["trsv"][1])
    if "ilu0" in src:
        return square_case("ilu0", src["ilu0"])
    if "randdiag" in src:
        seed, n, nnz = src["randdiag"]
        return (n, n) + rand_square(seed, n, nnz)
    if "graph" in src:                   # colourref.built_graphs(): a pattern; the values are never read by the graph routines
        n, I, J = colourref.built_graphs()[src["graph"]]
        return n, n, I, J, 0.5 + (np.arange(len(I)) % 5) * 0.25
    if "system" in src:                  # tests/amgcases.py's systems (krylovcases' spd_* and gen_*, poisson_40, diag_50)
        global _SYSTEMS
        if _SYSTEMS is None:
            import amgcases
            _SYSTEMS = amgcases.cases()
        n, I, J, V = _SYSTEMS[src["system"]][0]
        return n, n, np.asarray(I, np.int32), np.asarray(J, np.int32), np.asarray(V, np.float64)
    seed, rows, cols, nnz, clustered = src["rand"]
    return (rows, cols) + rand_matrix(seed, rows, cols, nnz, bool(clustered))


def values(shape, seed, special, dtype):
    """the values a record names by seed: standard normal, or with test_gpu_sddmm.py's _specials mix"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(shape)
    if special:
        sp = rng.random(v.shape) < 0.25
        v[sp] = rng.choice(SPECIAL, int(sp.sum()))
    return v.astype(dtype)


def dt(name):
    return np.dtype({"f64": np.float64, "f32": np.float32}[name])


def dtname(dtype):
    return "f32" if np.dtype(dtype) == np.float32 else "f64"


def rows_of(rows, rp):
    return np.repeat(np.arange(rows, dtype=np.int64), np.diff(np.asarray(rp, np.int64)))


def same(got, want, kind="exact"):
    """test_gpu_sddmm.py's _same: equal bits, NaN equals NaN, and +0 equals -0 only under min / max"""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    ok = (got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want))
    if kind == "minmax":
        ok |= (got == 0) & (want == 0)
    return bool(np.all(ok))


class MTiled:
    def __init__(self, rows, cols, dtype, rp, ci, vals, prov=None):
        self.rows, self.cols, self.dtype = int(rows), int(cols), np.dtype(dtype)
        self.rp, self.ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
        self.vals = np.ascontiguousarray(vals, self.dtype)
        self.vals_t = self.vals          # what the vals_t readers see (differs from vals only under the "stale_vals_t" mutation)
        self.version = 0
        self.prov = prov
        self.built = set()               # lazily built structures (coverage bookkeeping only)
        self.last_writer = None          # the last in-place writer kind (coverage bookkeeping only)
        self.trail = []                  # of a concat or a factor: refreshes, writes to a source, trim / reserve (coverage only)
        self.kept = {}                   # what a mutation of the second set holds on to (values as of some earlier call)

    @property
    def nnz(self):
        return len(self.ci)

    @property
    def tile_rows(self):
        return (self.rows + 15) // 16

    def coo(self):
        return rows_of(self.rows, self.rp), self.ci, self.vals

    @classmethod
    def from_coo(cls, rows, cols, I, J, V, dtype, prov=None):
        rp, ci, v = semiringref.coo_to_csr(rows, cols, I, J, np.asarray(V, dtype))
        return cls(rows, cols, dtype, rp, ci, v, prov)


class MPlan:
    def __init__(self, A, B, M, complement, lo, hi, semiring):
        self.A, self.B, self.M, self.complement, self.lo, self.hi, self.semiring = A, B, M, bool(complement), lo, hi, semiring
        self.options = dict(OPTION_DEFAULT)
        self.state = 0
        self.C = None                    # (rowptr, colidx, vals) of rows [row0, row1), as step 3 last left it
        self.c_versions, self.c_semiring = None, None
        self.passes = 0                  # completed pem_spgemm calls since the last option change (coverage bookkeeping only)
        self.option_epoch = 0
        self.trail = []                  # coverage bookkeeping only

    @property
    def row0(self):
        return 16 * self.lo

    @property
    def row1(self):
        return min(16 * self.hi, self.A.rows)


class MKrylov:
    """a pem_krylov: the ids of A and of its factor or hierarchy (handles, not copies), and the options of create"""

    def __init__(self, a, pre, method, precond, max_iters, check_every, rtol, atol):
        self.a, self.pre, self.method, self.precond = a, pre, method, precond
        self.max_iters, self.check_every, self.rtol, self.atol = int(max_iters), int(check_every), float(rtol), float(atol)
        self.kept = {}                   # the factor's values as of create (the "krylov_stale_factor" mutation)
        self.trail = []                  # coverage bookkeeping only


class MAmg:
    """a pem_amg: the id of A, the options of create, and amgref's levels as of the last create / refresh (level 0's matrix is A
    itself, a handle: Model.levels puts A's current values there)"""

    def __init__(self, a, opts, levels):
        self.a, self.opts, self.levels = a, dict(opts), levels
        self.stalled = False             # the aggregation returned naggregates == n (coverage bookkeeping only)
        self.trail = []                  # coverage bookkeeping only


def priority(n, spec):
    """the uint32 priorities of a graph record: ["seed", s] (the hash), ["equal", where] or ["ties", where] (test_gpu_colour.py's
    arrays; where: "host" / "device")"""
    return aggref.priority_array(n, spec[1] if spec[0] == "seed" else spec[0])


def graph_demand(kind, n):
    """bytes of the context's graph scratch a call of `kind` on n vertices carves (csrc: every part rounded up to 256 bytes)"""
    r = lambda b: (b + 255) & ~255
    return {"colour": r(4 * n) + r(12), "colour_order": 2 * r(8 * n) + 2 * r(4 * n), "components": 2 * r(4 * (n + 1)) + r(8),
            "mis": r(n) + r(8 * n) + r(4 * (n + 1)) + r(8), "aggregate": 2 * r(n) + r(8 * n) + 2 * r(4 * (n + 1)) + r(8)}[kind]


class Result:
    """what one record did: status; wrote = the id of the handle whose contents it (re)wrote, with the `kind` its values are
    compared under ("exact", or "minmax": +0 == -0); out = what the call returns to the caller (CSR / COO triple or dense array)"""

    def __init__(self, status=PEM_OK, wrote=None, kind="exact", out=None, extra=None):
        self.status, self.wrote, self.kind, self.out = status, wrote, kind, out
        self.extra = extra               # of a solve: what res->launches follows from (the runner adds the trsv launches of the device)


def _kind(name):
    return "minmax" if name in MINMAX or name in ("min", "max") else "exact"


def sources(prov):
    """the ids of the tilings a provenance tuple names (a concat's cells: the non-null ones, repeats included)"""
    if prov is None or prov[0] in ("cplan", "build"):
        return ()
    if prov[0] in ("ewise", "kron", "assign"):
        return (prov[1], prov[2])
    if prov[0] == "concat":
        return tuple(h for h in prov[1] if h is not None)
    return (prov[1],)


def triplets(a, dtype):
    """(rows, cols, I, J, V) of a build record's triplet list: the record's matrix with every entry repeated 1 to 5 times (mostly
    once) and, under a["long"], a few of them as often as or more often than the build folds strictly in order"""
    rows, cols, I, J, V = matrix(a["src"])
    rng = np.random.default_rng(a["lens_seed"])
    lengths = rng.choice(np.array([1, 1, 1, 2, 3, 5]), len(I))
    if a["long"] and len(I):
        lengths[rng.integers(0, len(I), 3)] = rng.choice(np.array([32, 33, 40]), 3)    # (BUILD_INORDER_MAX is 32)
    I2, J2, V2 = buildref.with_duplicates(I, J, np.asarray(V, dtype), rng, lengths)
    return rows, cols, I2, J2, V2


def symmetric(T):
    """a square tiling whose pattern equals its transpose's (what triangle_count takes)"""
    if T.rows != T.cols:
        return False
    I, J, _ = T.coo()
    return np.array_equal(np.sort(I * T.cols + J), np.sort(J * T.cols + I))


def index_list(spec, dim):
    """an index argument of extract as the records carry it: None (all), ["slice", start, stop, step], ["host", [..]] or
    ["device", [..]] -> None or the int64 list"""
    if spec is None:
        return None
    if spec[0] == "slice":
        return np.arange(*slice(*spec[1:]).indices(dim), dtype=np.int64)
    return np.asarray(spec[1], np.int64)


def missing_diag(T):
    """(rows without a stored diagonal entry, the first of them 1-based or 0) of a square tiling"""
    I, J, _ = T.coo()
    has = np.zeros(T.rows, bool)
    has[I[I == J]] = True
    miss = np.flatnonzero(~has)
    return len(miss), int(miss[0]) + 1 if len(miss) else 0


def ilu0_cost(T):
    """steps of ilu0ref's inner loop on T (the generator's size guard)"""
    return int((np.diff(T.rp) ** 2).sum())


def trsv_fields(T, uplo):
    """pem_tiled_trsv_info's levels, max_width, missing_diag, first_missing_row from trsvref.levels of the pattern"""
    w = trsvref.widths(trsvref.levels(T.rows, T.rp, T.ci, uplo))
    return np.array([len(w), max(w)] + list(missing_diag(T)), np.int64)


def pivot_fields(T):
    """pem_tiled_ilu0_info's zero_pivots and first_zero_pivot_row of a factor, by ilu0ref.pivots"""
    return np.array(ilu0ref.pivots(T.rows, T.rp, T.ci, T.vals), np.int64)


class Model:
    def __init__(self, mutations=()):
        assert all(m in MUTATIONS for m in mutations)
        self.mut = set(mutations)
        self.t, self.p = {}, {}
        self.k, self.h = {}, {}          # the third set's pools: solvers, hierarchies

    # ---- helpers -----------------------------------------------------------------------------------------------------------
    def current(self, p):
        return p.state == 3 and p.c_versions == (p.A.version, p.B.version) and p.c_semiring == p.semiring

    def _wrote(self, T, vals, writer):
        T.vals = np.ascontiguousarray(vals, T.dtype)
        if "stale_vals_t" not in self.mut:
            T.vals_t = T.vals
        if "no_bump" not in self.mut:
            T.version += 1
        T.last_writer = writer
        T.built.add("vmap_t")
        for p in self.p.values():
            if p.A is T or p.B is T:
                p.trail.append("refresh")
        for D in self.t.values():
            if D.prov is not None and D.prov[0] in ("concat", "ilu0") and any(self.t.get(h) is T for h in sources(D.prov)):
                D.trail.append("source")

    def adopt(self, tid, vals):
        """take the device's bits where the header leaves them open (the sign of a zero under min / max, NaN payloads)"""
        T = self.t[tid]
        same = T.vals_t is T.vals
        T.vals = np.ascontiguousarray(vals, T.dtype).copy()
        if same:
            T.vals_t = T.vals

    def product(self, p):
        """C of plan p from its operands' current values, by the references of the plan tests"""
        A, B = p.A, p.B
        f32 = A.dtype == np.float32
        if p.semiring == "plus_times":
            o = oracle()
            oa = o.Csr(A.rows, A.cols, rows_of(A.rows, A.rp), A.ci, A.vals.astype(np.float64))
            ob = o.Csr(B.rows, B.cols, rows_of(B.rows, B.rp), B.ci, B.vals.astype(np.float64))
            c = o.csr_spgemm(oa, ob, f32=f32)
            rp, ci, v = (np.array(x) for x in c.arrays())
            v = v.astype(A.dtype)
        else:
            rp, ci, v = semiringref.spgemm((A.rp, A.ci, A.vals), (B.rp, B.ci, B.vals), B.cols, p.semiring, A.dtype)
        rp = np.asarray(rp, np.int64)
        r0, r1 = p.row0, p.row1
        e0, e1 = int(rp[r0]), int(rp[r1])
        rp, ci, v = rp[r0:r1 + 1] - e0, np.asarray(ci)[e0:e1], np.asarray(v, A.dtype)[e0:e1]
        if p.M is not None:
            mi, mj, _ = p.M.coo()
            rp, ci, v = maskref.filter_csr(rp, ci, v, mi, mj, B.cols, p.complement, row0=r0)
        return np.asarray(rp, np.int32), np.asarray(ci, np.int32), np.ascontiguousarray(v, A.dtype)

    def products(self, A, B):
        """scalar products of A*B (the generator's size guard)"""
        return int(np.diff(B.rp)[A.ci].sum()) if A.nnz else 0

    def _step3(self, p):
        p.C = self.product(p)
        p.state = 3
        p.c_versions, p.c_semiring = (p.A.version, p.B.version), p.semiring

    # ---- one record ----------------------------------------------------------------------------------------------------------
    def apply(self, rec):
        op, ids, a = rec
        with np.errstate(all="ignore"):
            return getattr(self, "op_" + op)(ids, a)

    # tilings
    def _new(self, a, T):
        self.t[a["out"]] = T
        return Result(wrote=a["out"])

    def _converted(self, a, transpose):
        rows, cols, I, J, V = matrix(a["src"])
        if transpose:
            rows, cols, I, J = cols, rows, J, I
        return self._new(a, MTiled.from_coo(rows, cols, I, J, V, dt(a["dtype"])))

    def op_from_coo(self, ids, a):
        return self._converted(a, a["transpose"])

    def op_from_coo_device(self, ids, a):
        return self._converted(a, a["transpose"])

    def op_from_csr(self, ids, a):
        return self._converted(a, False)

    def op_close(self, ids, a):
        del self.t[ids[0]]
        return Result()

    def op_save_load(self, ids, a):
        T = self.t[ids[0]]
        return self._new(a, MTiled(T.rows, T.cols, T.dtype, T.rp, T.ci, T.vals.copy()))

    # plans
    def op_plan_create(self, ids, a):
        A, B = self.t[ids[0]], self.t[ids[1]]
        M = self.t[ids[2]] if ids[2] is not None else None
        hi = A.tile_rows if a["hi"] < 0 else a["hi"]
        self.p[a["out"]] = MPlan(A, B, M, a["complement"], a["lo"], hi, a["semiring"])
        return Result()

    def op_plan_close(self, ids, a):
        del self.p[ids[0]]
        return Result()

    def op_step1(self, ids, a):
        p = self.p[ids[0]]
        p.state = 1
        p.trail.append("step1")
        return Result()

    def op_step2(self, ids, a):
        p = self.p[ids[0]]
        if p.state < 1:
            return Result(PEM_E_STATE)
        p.state = 2
        p.trail.append("step2")
        return Result()

    def op_step3(self, ids, a):
        p = self.p[ids[0]]
        if p.state < 2:
            return Result(PEM_E_STATE)
        self._step3(p)
        p.trail.append("step3")
        return Result(wrote=ids[0], kind=_kind(p.semiring))

    def op_spgemm(self, ids, a):
        p = self.p[ids[0]]
        self._step3(p)
        p.trail.append("warm" if p.passes else "full")
        p.passes += 1
        return Result(wrote=ids[0], kind=_kind(p.semiring))

    def op_set_semiring(self, ids, a):
        self.p[ids[0]].semiring = a["semiring"]
        return Result()

    def op_set_option(self, ids, a):
        p = self.p[ids[0]]
        name, value = a["name"], a["value"]
        if p.M is not None and name == "wide" and value == 0:
            return Result(PEM_E_INVALID)
        v = int(value) if name in OPTION_INT else int(value != 0)
        if p.options[name] == v:
            return Result()
        p.options[name] = v
        p.passes = 0
        p.option_epoch += 1
        p.trail.append("option")
        if "no_option_reset" not in self.mut:
            p.state = min(p.state, OPTION_KEEP[name])
        return Result()

    def op_export_csr(self, ids, a):
        p = self.p[ids[0]]
        if not self.current(p):
            return Result(PEM_E_STATE)
        return Result(out=p.C, kind=_kind(p.semiring))

    def op_export_coo(self, ids, a):
        p = self.p[ids[0]]
        if not self.current(p):
            return Result(PEM_E_STATE)
        rp, ci, v = p.C
        return Result(out=((p.row0 + rows_of(len(rp) - 1, rp)).astype(np.int32), ci, v), kind=_kind(p.semiring))

    # derived tilings
    def _c_as_tiling(self, p, transpose, prov):
        rp, ci, v = p.C
        I = p.row0 + rows_of(len(rp) - 1, rp)
        A, B = p.A, p.B
        if transpose:
            return MTiled.from_coo(B.cols, A.rows, ci, I, v, A.dtype, prov)
        return MTiled.from_coo(A.rows, B.cols, I, ci, v, A.dtype, prov)

    def op_from_cplan(self, ids, a):
        p = self.p[ids[0]]
        if not self.current(p):
            return Result(PEM_E_STATE)
        return self._new(a, self._c_as_tiling(p, a["transpose"], ("cplan", ids[0], bool(a["transpose"]))))

    def op_set_values_from_cplan(self, ids, a):
        T, p = self.t[ids[0]], self.p[ids[1]]
        if T.prov is None or T.prov[0] != "cplan" or T.prov[1] != ids[1]:
            return Result(PEM_E_INVALID)
        if not self.current(p):
            return Result(PEM_E_STATE)
        if T.prov[2]:
            T.built.add("map_cplan")
        self._wrote(T, self._c_as_tiling(p, T.prov[2], None).vals, "from_cplan")
        return Result(wrote=ids[0])

    def _ewise(self, A, B, op, pattern, alpha, beta):
        ai, aj, av = A.coo()
        bi, bj, bv = B.coo()
        return ewiseref.ewise(A.cols, (ai, aj, av), (bi, bj, bv), op, pattern, alpha, beta)

    def op_ewise(self, ids, a):
        A, B = self.t[ids[0]], self.t[ids[1]]
        I, J, V = self._ewise(A, B, a["op"], a["pattern"], a["alpha"], a["beta"])
        r = self._new(a, MTiled.from_coo(A.rows, A.cols, I, J, V, A.dtype, ("ewise", ids[0], ids[1], a["op"], a["pattern"], a["alpha"], a["beta"])))
        r.kind = _kind(a["op"])
        return r

    def op_set_values_from_ewise(self, ids, a):
        T = self.t[ids[0]]
        if T.prov is None or T.prov[0] != "ewise" or (T.prov[1], T.prov[2]) != (ids[1], ids[2]):
            return Result(PEM_E_INVALID)
        _, _, V = self._ewise(self.t[ids[1]], self.t[ids[2]], *T.prov[3:])
        T.built.add("map_ewise")
        self._wrote(T, V, "from_ewise")
        return Result(wrote=ids[0], kind=_kind(T.prov[3]))

    def op_select(self, ids, a):
        A = self.t[ids[0]]
        I, J, V = selectref.select(*A.coo(), a["op"], a["thunk"], A.dtype)
        return self._new(a, MTiled.from_coo(A.rows, A.cols, I, J, V, A.dtype, ("select", ids[0], a["op"], a["thunk"])))

    def op_set_values_from_select(self, ids, a):
        T = self.t[ids[0]]
        if T.prov is None or T.prov[0] != "select" or T.prov[1] != ids[1] or T.prov[2] not in selectref.POSITIONAL:
            return Result(PEM_E_INVALID)
        _, _, V = selectref.select(*self.t[ids[1]].coo(), T.prov[2], T.prov[3], T.dtype)
        T.built.add("map_select")
        self._wrote(T, V, "from_select")
        return Result(wrote=ids[0])

    def sddmm_operands(self, S, a, dtype):
        """X (rows x k) and Y (cols x k) as column slices of wider buffers, as test_gpu_sddmm.py's _operands"""
        k = a["k"]
        Xw = values((S.rows, k + 3), a["seed"], a["special"], dtype)
        Yw = values((S.cols, k + 11), a["seed"] + 1, a["special"], dtype)
        return Xw, Yw, Xw[:, 2:2 + k], Yw[:, 5:5 + k]

    def op_sddmm(self, ids, a):
        S = self.t[ids[0]]
        dtype = dt(a["dtype"])
        _, _, X, Y = self.sddmm_operands(S, a, dtype)
        I, J, _ = S.coo()
        V = sddmmref.sddmm(I, J, X, Y, a["semiring"], dtype, oracle=oracle())
        r = self._new(a, MTiled(S.rows, S.cols, dtype, S.rp, S.ci, V))
        r.kind = _kind(a["semiring"])
        return r

    # value writers
    def op_set_values(self, ids, a):
        T = self.t[ids[0]]
        V = values(T.nnz, a["seed"], a["special"], T.dtype)
        if a["order"] == "col":          # V is in (col, row) order: position of every CSR entry in that order
            I, J, _ = T.coo()
            pos = np.empty(T.nnz, np.int64)
            pos[np.lexsort((I, J))] = np.arange(T.nnz)
            V = V[pos]
        T.built.add("vmap_" + a["order"])
        self._wrote(T, V, "set_values_" + a["order"])
        return Result(wrote=ids[0])

    def op_set_values_device(self, ids, a):
        return self.op_set_values(ids, a)

    def op_set_values_sddmm(self, ids, a):
        T = self.t[ids[0]]
        _, _, X, Y = self.sddmm_operands(T, a, T.dtype)
        I, J, old = T.coo()
        V = sddmmref.sddmm(I, J, X, Y, a["semiring"], T.dtype, old=old if a["accumulate"] else None, oracle=oracle())
        self._wrote(T, V, "sddmm_acc" if a["accumulate"] else "sddmm")
        return Result(wrote=ids[0], kind=_kind(a["semiring"]))

    # dense readers
    def op_mxv(self, ids, a):
        T = self.t[ids[0]]
        nx, ny = (T.rows, T.cols) if a["transpose"] else (T.cols, T.rows)
        x = values(nx, a["seed"], a["special"], T.dtype)
        y0 = values(ny, a["seed"] + 1, a["special"], T.dtype) if a["accumulate"] else None
        if a["transpose"]:
            T.built.add("mx_cols")
        y = mxvref.mxv(T.rows, T.cols, T.rp, T.ci, T.vals, x, a["semiring"], T.dtype, y0=y0, oracle=oracle(), transpose=a["transpose"])
        return Result(out=np.asarray(y, T.dtype), kind=_kind(a["semiring"]))

    def op_reduce(self, ids, a):
        T = self.t[ids[0]]
        ny = T.cols if a["dim"] == "cols" else T.rows
        y0 = values(ny, a["seed"] + 1, a["special"], T.dtype) if a["accumulate"] else None
        if a["dim"] == "cols":
            T.built.add("mx_cols")
        y = mxvref.reduce(T.rows, T.cols, T.rp, T.ci, T.vals, a["op"], T.dtype, y0=y0, dim=a["dim"])
        return Result(out=np.asarray(y, T.dtype), kind=_kind(a["op"]))

    def spmm_operands(self, T, a):
        """X as a column slice of a wider buffer, Y as the first k columns of one"""
        k = a["k"]
        nx, ny = (T.rows, T.cols) if a["transpose"] else (T.cols, T.rows)
        Xw = values((nx, k + 3), a["seed"], a["special"], T.dtype)
        Yfull = values((ny, k + 2), a["seed"] + 1, a["special"], T.dtype)
        return Xw, Yfull

    def op_spmm(self, ids, a):
        T = self.t[ids[0]]
        k = a["k"]
        Xw, Yfull = self.spmm_operands(T, a)
        if a["transpose"]:
            T.built.add("mx_cols")
        Y = spmmref.spmm_into(T.rows, T.cols, T.rp, T.ci, T.vals, Xw[:, 1:1 + k], Yfull, k, a["semiring"], T.dtype, accumulate=a["accumulate"],
                              oracle=oracle(), transpose=a["transpose"])
        return Result(out=Y, kind=_kind(a["semiring"]))

    # ---- the second operation set: derived tilings with a refresh --------------------------------------------------------------
    def _made_from(self, T, kind, srcs):
        """the serial rule of the set_values_from_* calls: T was made by `kind` from exactly these tilings, in this order"""
        if T.prov is None or T.prov[0] != kind:
            return False
        return tuple(T.prov[1]) == tuple(srcs) if kind == "concat" else sources(T.prov) == tuple(srcs)

    def _refreshed(self, ids, kind, V, result_kind="exact", built=None):
        T = self.t[ids[0]]
        if built:
            T.built.add(built)
        T.trail.append("refresh")
        self._wrote(T, V, "from_" + kind)
        return Result(wrote=ids[0], kind=result_kind)

    def op_apply(self, ids, a):
        A = self.t[ids[0]]
        if a["op"] == "powi" and not applyref.powi_thunk_ok(a["thunk"]):
            return Result(PEM_E_INVALID)
        V = applyref.apply(A.vals, a["op"], a["thunk"], A.dtype)
        r = self._new(a, MTiled(A.rows, A.cols, A.dtype, A.rp, A.ci, V, ("apply", ids[0], a["op"], a["thunk"])))
        r.kind = _kind(a["op"])
        return r

    def op_set_values_from_apply(self, ids, a):
        T = self.t[ids[0]]
        if not self._made_from(T, "apply", ids[1:]):
            return Result(PEM_E_INVALID)
        return self._refreshed(ids, "apply", applyref.apply(self.t[ids[1]].vals, T.prov[2], T.prov[3], T.dtype), _kind(T.prov[2]))

    def _scaled(self, A, a, op):
        """a["rows"] / a["cols"]: the seed of that vector, or None"""
        r, c = (None if a[k] is None else values(n, a[k], a["special"], A.dtype) for k, n in (("rows", A.rows), ("cols", A.cols)))
        I, J, V = A.coo()
        return applyref.scale(I, J, V, r, c, op, A.dtype)

    def op_scale(self, ids, a):
        A = self.t[ids[0]]
        r = self._new(a, MTiled(A.rows, A.cols, A.dtype, A.rp, A.ci, self._scaled(A, a, a["op"]), ("scale", ids[0], a["op"])))
        r.kind = _kind(a["op"])
        return r

    def op_set_values_from_scale(self, ids, a):
        T = self.t[ids[0]]
        if not self._made_from(T, "scale", ids[1:]):
            return Result(PEM_E_INVALID)
        return self._refreshed(ids, "scale", self._scaled(self.t[ids[1]], a, T.prov[2]), _kind(T.prov[2]))

    def _assigned(self, C, A, rows, cols, accum, prov=None):
        I, J, V = assignref.assign(C.rows, C.cols, C.coo(), A.coo(), index_list(rows, C.rows), index_list(cols, C.cols), accum)
        return MTiled.from_coo(C.rows, C.cols, I, J, V, C.dtype, prov)

    def op_assign(self, ids, a):
        C, A = self.t[ids[0]], self.t[ids[1]]
        for spec in (a["rows"], a["cols"]):
            if spec is not None and spec[0] != "slice" and len(set(spec[1])) != len(spec[1]):
                return Result(PEM_E_INVALID)
        r = self._new(a, self._assigned(C, A, a["rows"], a["cols"], a["accum"], ("assign", ids[0], ids[1], a["rows"], a["cols"], a["accum"])))
        r.kind = _kind(a["accum"])
        return r

    def op_set_values_from_assign(self, ids, a):
        T = self.t[ids[0]]
        if not self._made_from(T, "assign", ids[1:]):
            return Result(PEM_E_INVALID)
        V = self._assigned(self.t[ids[1]], self.t[ids[2]], *T.prov[3:]).vals
        return self._refreshed(ids, "assign", V, _kind(T.prov[5]), "map_assign")

    def op_build(self, ids, a):
        dtype = dt(a["dtype"])
        rows, cols, I, J, V = triplets(a, dtype)
        oI, oJ, oV = buildref.fold(rows, cols, I, J, V, a["dup"], a["transpose"])
        if a["transpose"]:
            rows, cols = cols, rows
        prov = ("build", {k: a[k] for k in ("src", "lens_seed", "long", "dup", "transpose", "keep_map")}, len(I))
        r = self._new(a, MTiled.from_coo(rows, cols, oI, oJ, oV, dtype, prov))
        r.kind = _kind(a["dup"])
        return r

    def op_build_device(self, ids, a):
        return self.op_build(ids, a)

    def op_set_values_from_build(self, ids, a):
        T = self.t[ids[0]]
        if T.prov is None or T.prov[0] != "build" or not T.prov[1]["keep_map"] or a["nnz_in"] != T.prov[2]:
            return Result(PEM_E_INVALID)
        b = T.prov[1]
        rows, cols, I, J, _ = triplets(b, T.dtype)
        _, _, V = buildref.fold(rows, cols, I, J, values(len(I), a["seed"], a["special"], T.dtype), b["dup"], b["transpose"])
        return self._refreshed(ids, "build", V, _kind(b["dup"]), "map_build")

    def _sampled(self, S, A, B, a, old=None):
        if a["transpose_b"]:
            B = self._transposed(B)
        I, J, _ = S.coo()
        return sampledref.sampled(I, J, (A.rp, A.ci, A.vals), (B.rp, B.ci, B.vals), A.cols, B.cols, a["semiring"], A.dtype, old, oracle())

    def op_sampled_mxm(self, ids, a):
        S, A, B = (self.t[h] for h in ids)
        r = self._new(a, MTiled(S.rows, S.cols, A.dtype, S.rp, S.ci, self._sampled(S, A, B, a)))
        r.kind = _kind(a["semiring"])
        return r

    def op_set_values_sampled_mxm(self, ids, a):
        T, A, B = (self.t[h] for h in ids)
        self._wrote(T, self._sampled(T, A, B, a, T.vals if a["accumulate"] else None), "sampled_acc" if a["accumulate"] else "sampled")
        return Result(wrote=ids[0], kind=_kind(a["semiring"]))

    def op_triangle_count(self, ids, a):
        T = self.t[ids[0]]
        I, J, _ = T.coo()
        off = I != J                             # (the diagonal is not read)
        return Result(out=np.array([sampledref.triangles(T.rows, I[off], J[off])], np.int64))

    def op_select_topk(self, ids, a):
        A = self.t[ids[0]]
        if a["dim"] == "cols":
            A.built.add("mx_cols")
        I, J, V = topkref.select_topk(*A.coo(), a["order"], a["dim"], a["k"], A.dtype)
        return self._new(a, MTiled.from_coo(A.rows, A.cols, I, J, V, A.dtype))

    def _transposed(self, A, prov=None):
        rows, cols, I, J, V = extractref.transpose(A.rows, A.cols, *A.coo())
        return MTiled.from_coo(rows, cols, I, J, V, A.dtype, prov)

    def op_transpose(self, ids, a):
        return self._new(a, self._transposed(self.t[ids[0]], ("transpose", ids[0])))

    def op_set_values_from_transpose(self, ids, a):
        if not self._made_from(self.t[ids[0]], "transpose", ids[1:]):
            return Result(PEM_E_INVALID)
        return self._refreshed(ids, "transpose", self._transposed(self.t[ids[1]]).vals, built="map_transpose")

    def _extracted(self, A, rows, cols, prov=None):
        ni, nj, I, J, V = extractref.extract(A.rows, A.cols, *A.coo(), index_list(rows, A.rows), index_list(cols, A.cols))
        return MTiled.from_coo(ni, nj, I, J, V, A.dtype, prov)

    def op_extract(self, ids, a):
        for spec in (a["rows"], a["cols"]):
            if spec is not None and spec[0] != "slice" and len(spec[1]) == 0:
                return Result(PEM_E_INVALID)
        return self._new(a, self._extracted(self.t[ids[0]], a["rows"], a["cols"], ("extract", ids[0], a["rows"], a["cols"])))

    def op_set_values_from_extract(self, ids, a):
        T = self.t[ids[0]]
        if not self._made_from(T, "extract", ids[1:]):
            return Result(PEM_E_INVALID)
        return self._refreshed(ids, "extract", self._extracted(self.t[ids[1]], T.prov[2], T.prov[3]).vals, built="map_extract")

    def _kron(self, A, B, op, prov=None):
        rows, cols, I, J, V = kronref.kron(A.rows, A.cols, *A.coo(), B.rows, B.cols, *B.coo(), op, A.dtype)
        return MTiled.from_coo(rows, cols, I, J, V, A.dtype, prov)

    def op_kron(self, ids, a):
        r = self._new(a, self._kron(self.t[ids[0]], self.t[ids[1]], a["op"], ("kron", ids[0], ids[1], a["op"])))
        r.kind = _kind(a["op"])
        return r

    def op_set_values_from_kron(self, ids, a):
        T = self.t[ids[0]]
        if not self._made_from(T, "kron", ids[1:]):
            return Result(PEM_E_INVALID)
        return self._refreshed(ids, "kron", self._kron(self.t[ids[1]], self.t[ids[2]], T.prov[3]).vals, _kind(T.prov[3]), "map_kron")

    @staticmethod
    def _grid(flat, gc):
        return [list(flat[k:k + gc]) for k in range(0, len(flat), gc)]

    def op_concat(self, ids, a):
        gr, gc = a["grid"]
        blocks = self._grid([None if h is None else self.t[h].coo() for h in ids], gc)
        rows, cols, I, J, V = concatref.concat(blocks, a["row_sizes"], a["col_sizes"], dt(a["dtype"]))
        prov = ("concat", tuple(ids), gc, tuple(a["row_sizes"]), tuple(a["col_sizes"]))
        return self._new(a, MTiled.from_coo(rows, cols, I, J, V, dt(a["dtype"]), prov))

    def op_set_values_from_concat(self, ids, a):
        T = self.t[ids[0]]
        if not self._made_from(T, "concat", ids[1:]):
            return Result(PEM_E_INVALID)
        cells = [None if h is None else self.t[h] for h in T.prov[1]]
        values = [None if c is None else c.vals for c in cells]
        if "concat_stale_block" in self.mut:     # (the blocks' values as of the first refresh: a pointer table never rewritten)
            values = T.kept.setdefault("blocks", values)
        blocks = self._grid([None if c is None else c.coo() for c in cells], T.prov[2])
        return self._refreshed(ids, "concat", concatref.refreshed(blocks, T.prov[3], T.prov[4], values, T.dtype), built="map_concat")

    def op_ilu0(self, ids, a):
        A = self.t[ids[0]]
        if A.rows != A.cols or missing_diag(A)[0]:
            return Result(PEM_E_INVALID)
        V, _ = ilu0ref.ilu0(A.rows, A.rp, A.ci, A.vals, A.dtype)
        F = MTiled(A.rows, A.cols, A.dtype, A.rp, A.ci, V, ("ilu0", ids[0]))
        F.kept["source"] = A.vals
        F.trail.append("ilu0")
        self._schedule(F, "lower")               # (a factor is born with its lower schedule)
        return self._new(a, F)

    def op_set_values_from_ilu0(self, ids, a):
        F = self.t[ids[0]]
        if not self._made_from(F, "ilu0", ids[1:]):
            return Result(PEM_E_INVALID)
        A = self.t[ids[1]]
        src = F.kept["source"] if "ilu0_stale_source" in self.mut else A.vals
        return self._refreshed(ids, "ilu0", ilu0ref.ilu0(A.rows, A.rp, A.ci, src, A.dtype)[0])

    # ---- the second operation set: readers ---------------------------------------------------------------------------------------
    def _schedule(self, T, uplo):
        if "trsv_" + uplo not in T.built:
            T.built.add("trsv_" + uplo)
            T.kept[uplo] = T.vals

    def _trsv(self, T, b, uplo, unit_diag):
        self._schedule(T, uplo)
        vals = T.kept[uplo] if "trsv_stale_values" in self.mut else T.vals
        return trsvref.trsv(T.rows, T.rp, T.ci, vals, b, uplo, unit_diag, T.dtype)

    def op_trsv(self, ids, a):
        T = self.t[ids[0]]
        if T.rows != T.cols or a.get("overlap") or (not a["unit_diag"] and missing_diag(T)[0]):
            return Result(PEM_E_INVALID)
        return Result(out=self._trsv(T, values(T.rows, a["seed"], a["special"], T.dtype), a["uplo"], a["unit_diag"]))

    def op_lu_solve(self, ids, a):
        F = self.t[ids[0]]
        F.trail.append("lu_solve")
        work = self._trsv(F, values(F.rows, a["seed"], a["special"], F.dtype), "lower", True)
        return Result(out=self._trsv(F, work, "upper", False))

    def op_trsv_info(self, ids, a):
        T = self.t[ids[0]]
        self._schedule(T, a["uplo"])
        return Result(out=trsv_fields(T, a["uplo"]))

    def op_ilu0_info(self, ids, a):
        return Result(out=pivot_fields(self.t[ids[0]]))

    def frontier_operands(self, T, a):
        """x, the old out, the old index vector, x_present and mask of a frontier or arg record (None where the record has none):
        the absent x positions hold the special mix whatever the record says, the presence bytes are 0 / 1 / 255"""
        nx, ny = (T.rows, T.cols) if a["transpose"] else (T.cols, T.rows)
        rng = np.random.default_rng(a["seed"] + 2)
        present = {"none": None, "sparse": (rng.random(nx) < 0.3) * rng.choice(np.array([1, 255], np.uint8), nx),
                   "empty": np.zeros(nx, np.uint8)}[a["x_present"]]
        mask = None if a["mask"] is None else ((rng.random(ny) < 0.5) * rng.choice(np.array([1, 255], np.uint8), ny)).astype(np.uint8)
        x = None if a.get("x_none") else values(nx, a["seed"], a["special"], T.dtype)
        if x is not None and present is not None:
            x = np.where(present != 0, x, values(nx, a["seed"] + 3, True, T.dtype))
        idx0 = rng.integers(-1, max(nx, 1), ny).astype(np.int32)
        return x, values(ny, a["seed"] + 1, a["special"], T.dtype), idx0, None if present is None else present.astype(np.uint8), mask

    def op_mxv_frontier(self, ids, a):
        T = self.t[ids[0]]
        x, y0, _, present, mask = self.frontier_operands(T, a)
        if a["transpose"]:
            T.built.add("mx_cols")
        y, pres = frontierref.mxv_frontier(T.rows, T.cols, T.rp, T.ci, T.vals, x, a["semiring"], T.dtype, present, mask, a["mask"] == "complement",
                                           y_old=y0, accumulate=a["accumulate"], oracle=oracle(), transpose=a["transpose"])
        return Result(out=(np.asarray(y, T.dtype), pres) if a["out_present"] else np.asarray(y, T.dtype), kind=_kind(a["semiring"]))

    def op_mxv_arg(self, ids, a):
        T = self.t[ids[0]]
        x, y0, idx0, present, mask = self.frontier_operands(T, a)
        if a["transpose"]:
            T.built.add("mx_cols")
        y, idx, pres = argref.mxv_arg(T.rows, T.cols, T.rp, T.ci, T.vals, x, a["kind"], T.dtype, present, mask, a["mask"] == "complement",
                                      y_old=y0, idx_old=idx0, accumulate=a["accumulate"], transpose=a["transpose"])
        out = (() if y is None else (np.asarray(y, T.dtype),)) + (idx,) + ((pres,) if a["out_present"] else ())
        return Result(out=out, kind="minmax")

    def op_reduce_arg(self, ids, a):
        T = self.t[ids[0]]
        if a["dim"] == "cols":
            T.built.add("mx_cols")
        y, idx = argref.reduce_arg(T.rows, T.cols, T.rp, T.ci, T.vals, a["op"], T.dtype, a["dim"])
        return Result(out=(np.asarray(y, T.dtype), idx), kind="minmax")

    def op_bfs(self, ids, a):
        T = self.t[ids[0]]
        levels, depth, reached = frontierref.bfs(T.rows, T.rp, T.ci, a["source"], a["transpose"])
        return Result(out=(levels, np.array([depth, reached], np.int64)))

    def op_bfs_parents(self, ids, a):
        T = self.t[ids[0]]
        levels, parents, depth, reached = argref.bfs_parents(T.rows, T.rp, T.ci, a["source"], a["transpose"])
        return Result(out=(levels, parents, np.array([depth, reached], np.int64)))

    # ---- the third operation set: graph routines ---------------------------------------------------------------------------------
    def _graph(self, T, a):
        """(n, I, J, priorities) of a graph record, or None where the header refuses it; symmetric = 0 builds the column schedule"""
        if T.rows != T.cols or a.get("overlap"):
            return None
        if not a["symmetric"]:
            T.built.add("mx_cols")
        I, J, _ = T.coo()
        return T.rows, I, J, priority(T.rows, a["prio"]) if "prio" in a else None

    def _colouring(self, n, I, J, prio, symmetric):
        if "colour_ties_high" in self.mut:       # (ties to the higher index: the mirrored graph's colouring, mirrored back)
            c, nc, rounds = colourref.colouring(n, n - 1 - I, n - 1 - J, priority=prio[::-1], symmetric=symmetric)
            return c[::-1].copy(), nc, rounds
        return colourref.colouring(n, I, J, priority=prio, symmetric=symmetric)

    def op_colour(self, ids, a):
        g = self._graph(self.t[ids[0]], a)
        if g is None:
            return Result(PEM_E_INVALID)
        c, nc, rounds = self._colouring(*g, a["symmetric"])
        return Result(out=(c, np.array([nc, rounds], np.int64)))

    def op_components(self, ids, a):
        g = self._graph(self.t[ids[0]], a)
        if g is None:
            return Result(PEM_E_INVALID)
        labels, rounds = ccref.components_model(g[0], g[1], g[2], symmetric_walk=a["symmetric"])
        cid, nc = ccref.ids_of(labels)
        return Result(out=(labels,) + ((cid,) if a["ids"] else ()) + (np.array([nc, rounds], np.int64),))

    def op_colour_order(self, ids, a):
        """the keys (a colouring, or the component ids with ncolours = ncomponents) and their stable order"""
        g = self._graph(self.t[ids[0]], a)
        if a["of"] == "colour":
            keys, nk, _ = self._colouring(*g, a["symmetric"])
        else:
            keys, nk = ccref.ids_of(ccref.components_model(g[0], g[1], g[2], symmetric_walk=a["symmetric"])[0])
        perm = np.argsort(keys, kind="stable").astype(np.int32)
        offsets = np.concatenate([[0], np.cumsum(np.bincount(keys, minlength=nk))]).astype(np.int32)
        return Result(out=(np.asarray(keys, np.int32), perm, offsets, np.array([nk], np.int64)))

    def op_mis(self, ids, a):
        g = self._graph(self.t[ids[0]], a)
        if g is None or a["distance"] not in (1, 2):
            return Result(PEM_E_INVALID)
        s, count, rounds = aggref.mis(g[0], g[1], g[2], a["distance"], priority=g[3], symmetric=a["symmetric"])
        return Result(out=(s, np.array([count, rounds], np.int64)))

    def op_aggregate(self, ids, a):
        g = self._graph(self.t[ids[0]], a)
        if g is None:
            return Result(PEM_E_INVALID)
        agg, roots, nc, rounds = aggref.aggregate(g[0], g[1], g[2], priority=g[3], symmetric=a["symmetric"])
        return Result(out=(agg,) + ((roots,) if a["roots"] else ()) + (np.array([nc, rounds], np.int64),))

    # ---- the third operation set: solvers ------------------------------------------------------------------------------------------
    def op_krylov_create(self, ids, a):
        A = self.t[ids[0]]
        pre, pc = ids[1], a["precond"]
        F = self.t.get(pre) if pc != "amg" else None
        if A.rows != A.cols or (pc == "lu") != (F is not None) or (pc != "amg" and pre is not None and F is None):
            return Result(PEM_E_INVALID)
        if F is not None and ((F.rows, F.cols) != (A.rows, A.cols) or F.dtype != A.dtype or missing_diag(F)[0]):
            return Result(PEM_E_INVALID)
        if pc == "amg" and self.t.get(self.h[pre].a) is not A:
            return Result(PEM_E_INVALID)
        K = MKrylov(ids[0], pre, a["method"], pc, a["max_iters"], a["check_every"], a["rtol"], a["atol"])
        if F is not None:
            self._schedule(F, "lower")
            self._schedule(F, "upper")
            K.kept["factor"] = F.vals
        self.k[a["out"]] = K
        return Result()

    def solve_operands(self, n, a, dtype):
        """b, the guess (zeros where the record draws none) and the DIAG preconditioner's minv of a solve record"""
        b = values(n, a["seed"], a["special"], dtype)
        x0 = (0.1 * values(n, a["seed"] + 1, False, np.float64)).astype(dtype) if a["x0"] else np.zeros(n, dtype)
        return b, x0, (0.5 + np.abs(values(n, a["seed"] + 2, False, np.float64))).astype(dtype)

    def _solve(self, K, a):
        A = self.t[K.a]
        b, x0, minv = self.solve_operands(A.rows, a, A.dtype)
        opt = dict(method=K.method, max_iters=K.max_iters, rtol=K.rtol, atol=K.atol)
        if K.precond == "amg":
            H = self.h[K.pre]
            r = amgref.solve(self.levels(H), b, x0, oracle(), sweeps=H.opts["sweeps"], coarse_sweeps=H.opts["coarse_sweeps"], **opt)
        else:
            factor = None
            if K.precond == "lu":
                F = self.t[K.pre]
                factor = (F.rp, F.ci, K.kept["factor"] if "krylov_stale_factor" in self.mut else F.vals)
            r = krylovref.solve(A.rows, A.rp, A.ci, A.vals, b, x0, precond=K.precond, minv=minv if K.precond == "diag" else None, factor=factor,
                                dtype=A.dtype, oracle=oracle(), **opt)
        K.trail.append(krylovref.STATUS[r["status"]])
        ints = np.array([r["iters"], r["status"], krylovref.readbacks(r["stop_iter"], K.check_every)], np.int64)
        out = (np.asarray(r["x"], A.dtype), ints, np.array([r["bb"], r["rr"], r["threshold"]], np.float64))
        if a["history"]:
            out += (np.asarray(r["history"], np.float64),)
        return Result(out=out, extra=dict(method=K.method, precond=K.precond, stop_iter=r["stop_iter"], check_every=K.check_every,
                                          max_iters=K.max_iters, pre=K.pre))

    def op_krylov_solve(self, ids, a):
        if a.get("wrong_form"):                  # the fp64 entry point on an fp32 solver
            return Result(PEM_E_INVALID)
        return self._solve(self.k[ids[0]], a)

    def op_krylov_close(self, ids, a):
        del self.k[ids[0]]
        return Result()

    def op_tiled_solve(self, ids, a):
        """Tiled.solve: a solver made, used and closed in one call; precond "ilu0" makes and closes its own factor"""
        A = self.t[ids[0]]
        K = MKrylov(ids[0], None, a["method"], "lu" if a["precond"] == "ilu0" else "none", a["max_iters"], a["check_every"], a["rtol"], a["atol"])
        if a["precond"] == "ilu0":
            K.pre = "~factor"
            self.t[K.pre] = MTiled(A.rows, A.cols, A.dtype, A.rp, A.ci, ilu0ref.ilu0(A.rows, A.rp, A.ci, A.vals, A.dtype)[0])
            K.kept["factor"] = self.t[K.pre].vals
        try:
            r = self._solve(K, a)
        finally:
            self.t.pop("~factor", None)
        r.extra["trail"] = K.trail
        return r

    # ---- the third operation set: hierarchies ----------------------------------------------------------------------------------------
    def _hierarchy(self, A, o):
        I, J, V = A.coo()
        return amgref.hierarchy((A.rows, I, J, V), A.dtype, oracle(), smooth=o["smooth"], symmetric=o["symmetric"], seed=0,
                                max_levels=amgref.MAX_LEVELS, coarse_size=o["coarse_size"], omega=AMG_OMEGA)

    def levels(self, H):
        """H's levels as the device holds them now: level 0's matrix is A itself, with its current values"""
        A = self.t[H.a]
        first = dict(H.levels[0], A=(A.rows, A.cols, A.rp, A.ci, A.vals))
        return [first] + H.levels[1:]

    def op_amg_create(self, ids, a):
        A = self.t[ids[0]]
        if A.rows != A.cols or missing_diag(A)[0]:
            return Result(PEM_E_INVALID)
        H = MAmg(ids[0], a, self._hierarchy(A, a))
        last = H.levels[-1]["A"][0]
        H.stalled = len(H.levels) < amgref.MAX_LEVELS and last > a["coarse_size"]
        if not a["symmetric"] and (len(H.levels) > 1 or H.stalled):      # (pem_tiled_aggregate ran on A itself: its column schedule)
            A.built.add("mx_cols")
        H.trail.append("create")
        self.h[a["out"]] = H
        return Result()

    def op_amg_refresh(self, ids, a):
        H = self.h[ids[0]]
        if not H.opts["refreshable"]:
            return Result(PEM_E_STATE)
        new = self._hierarchy(self.t[H.a], H.opts)
        if "amg_stale_weights" in self.mut:      # (the weights of levels >= 1 stay as they were)
            for old, L in list(zip(H.levels, new))[1:]:
                L["w"] = old["w"]
        H.levels = new
        H.trail.append("refresh")
        return Result()

    def op_amg_apply(self, ids, a):
        H = self.h[ids[0]]
        A = self.t[H.a]
        H.trail.append("apply")
        z = amgref.apply(self.levels(H), values(A.rows, a["seed"], a["special"], A.dtype), oracle(), H.opts["sweeps"], H.opts["coarse_sweeps"])
        return Result(out=np.asarray(z, A.dtype))

    def amg_fields(self, H):
        """pem_amg_info's fields, bytes apart, in one array: levels, launches, then rows, nnz, p_nnz, aggregate_rounds of every level"""
        i = amgref.info(self.levels(H), H.opts["sweeps"], H.opts["coarse_sweeps"])
        return np.array([i["levels"], i["launches"]] + i["rows"] + i["nnz"] + i["p_nnz"] + i["aggregate_rounds"], np.int64)

    def op_amg_info(self, ids, a):
        self.h[ids[0]].trail.append("info")
        return Result(out=self.amg_fields(self.h[ids[0]]))

    def level_tiling(self, H, level, which):
        rows, cols, rp, ci, v = self.levels(H)[level][which]
        return MTiled(rows, cols, self.t[H.a].dtype, rp, ci, v)

    def op_amg_level(self, ids, a):
        """a borrowed A_l, P_l or R_l handed to a reader: a["reader"] is the reader's record without its handle"""
        H = self.h[ids[0]]
        op, args = a["reader"]
        T = self.level_tiling(H, a["level"], a["which"])
        if op == "export_csr":
            return Result(out=(np.asarray(T.rp, np.int32), np.asarray(T.ci, np.int32), T.vals))
        self.t["~level"] = T
        try:
            return self.apply((op, ("~level",), args))
        finally:
            del self.t["~level"]

    def op_amg_close(self, ids, a):
        del self.h[ids[0]]
        return Result()

    # housekeeping: nothing a caller can observe changes
    def _ctx_event(self):
        for T in self.t.values():
            if T.prov is not None and T.prov[0] == "concat":
                T.trail.append("ctx")

    def op_trim(self, ids, a):
        self._ctx_event()
        return Result()

    def op_reserve(self, ids, a):
        self._ctx_event()
        return Result()

    def op_synchronize(self, ids, a):
        return Result()
