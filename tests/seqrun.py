"""Runner of the sequence test: executes a program of tests/seqgen.py step by step on the GPU and on the host model of
tests/seqmodel.py, and compares after every step (tests/test_gpu_seq.py drives it, tools/seq_replay.py replays one program).

After every step:
  - a refusal the model predicts must come back as PemError with exactly that status, and the handles the call named are audited;
  - a call the model accepts must succeed;
  - the handle the step wrote is compared in full: a tiling by export_csr() (structure exact, values by `same`: equal bits, NaN equals
    NaN, +0 equals -0 only under min / max), a plan whose C is current by export_csr() alike, a dense result element for element.
Every AUDIT_EVERY steps and at the end, every live handle is audited (audit_tiling, audit_plan, audit_hierarchy): the damage this suite looks for is
to a handle the step did not name.  There is no tolerance anywhere and no entry is left out.

Where the header leaves bits open (the sign of a zero under min / max, NaN payloads) the model adopts the device's bits after the
comparison under that rule has passed, so that everything computed from them later is compared exactly again.

The third operation set (graph routines, solvers, hierarchies): every output buffer holds a poison value before the call; of a solve
the history past iters must still hold it.  Solvers and hierarchies go through the Python classes, as the feature tests call them;
the four refusals those classes cannot express (mis at distance 3, lu without a factor, a factor under another preconditioner, the
fp64 solve on an fp32 solver) call the C entry points.  _graph_call holds the graph scratch's allocation rule.

A mismatch raises SeqMismatch; its message carries the seed, the step, the failing record and the program up to that step in the
text form tools/seq_replay.py reads.  A HIP error status (PEM_E_HIP) raises SeqGpuError, after which nothing more is run.
"""
import ctypes as C

import numpy as np
import torch

import argref
import krylovref
import seqgen as sg
import seqmodel as sm
from semiringref import coo_to_csr
from seqmodel import same

AUDIT_EVERY = 10
PEM_E_HIP = -5
INFO = ("rows", "cols", "nnz", "tile_rows", "tile_cols", "ntiles", "value_bytes")
ARRAYS = ("tile_keys", "tile_nnz_ptr", "masks", "rowptr", "rowcolidx", "vals", "masks_t", "tile_rowptr", "tile_colidx", "tile_colptr",
          "tile_rowidx", "tile_offsets")
TRSV_FIELDS = ("levels", "max_width", "missing_diag", "first_missing_row")       # of pem_tiled_trsv_info; sm.trsv_fields' order
PIVOT_FIELDS = ("zero_pivots", "first_zero_pivot_row")                           # of pem_tiled_ilu0_info; sm.pivot_fields' order
SYMBOLIC = ("c_tile_rowptr", "c_tile_colidx", "c_mask", "c_tile_nnz_ptr")
POISON_I, POISON_B, POISON_F = -77777, 7, -7.25      # what every output buffer of the third set holds before the call


class SeqMismatch(AssertionError):
    def __init__(self, seed, step, where, rec, prog, what):
        self.seed, self.step, self.where, self.rec, self.what = seed, step, where, rec, what
        text = sg.dumps(prog[:step + 1])
        super().__init__(f"sequence mismatch: seed {seed}, step {step} ({where}): {what}\nrecord: {sg.dumps([rec]) if rec else '-'}\n"
                         f"program up to that step (tools/seq_replay.py reads it back):\n{text}")


class SeqGpuError(RuntimeError):
    pass


class Runner:
    """one context's pool on the device next to the model.  on_stream: the context works on torch's current stream, so torch
    tensors and the library's calls need no synchronisation between them; otherwise the runner synchronises both ways."""

    def __init__(self, pkg, ctx, tmpdir, on_stream=False, mutations=(), log=None):
        self.pkg, self.ctx, self.tmpdir, self.on_stream, self.log = pkg, ctx, str(tmpdir), on_stream, log
        self.m = sm.Model(mutations)
        self.t, self.p = {}, {}
        self.k, self.h = {}, {}          # the third set's pools: solvers, hierarchies
        self.res, self.pre_built = None, {}
        self.keep = []                   # device tensors a stream-ordered call may still read
        self.snap = {}                   # plan id -> (option epoch, symbolic arrays) of the last audit
        self.dense_a = {}
        self.seed, self.step, self.rec, self.prog = None, -1, None, []
        self.audits = 0

    # ---- plumbing -------------------------------------------------------------------------------------------------------------
    def fail(self, what, where="step"):
        raise SeqMismatch(self.seed, self.step, where, self.rec, self.prog, what)

    def dev(self, a):
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.keep.append(t)
        return t

    def uploaded(self):
        if not self.on_stream:
            torch.cuda.synchronize()

    def host(self, t):
        if not self.on_stream:
            self.ctx.synchronize()
        torch.cuda.synchronize()
        return t.cpu().numpy()

    def close(self):
        for k in self.k.values():
            k.close()
        for h in self.h.values():
            h.close()
        self.k, self.h = {}, {}
        for p in self.p.values():
            p.close()
        for t in self.t.values():
            t.close()
        for t in self.dense_a.values():
            t.close()
        self.p, self.t, self.dense_a = {}, {}, {}

    # ---- comparisons ------------------------------------------------------------------------------------------------------------
    def check_tiling(self, tid, kind="exact", where="step"):
        T, M = self.t[tid], self.m.t[tid]
        if (T.rows, T.cols, T.nnz, T.dtype) != (M.rows, M.cols, M.nnz, M.dtype):
            self.fail(f"{tid}: shape / nnz / dtype {(T.rows, T.cols, T.nnz, T.dtype)}, the model has {(M.rows, M.cols, M.nnz, M.dtype)}", where)
        rp, ci, v = T.export_csr()
        if not (np.array_equal(rp, M.rp) and np.array_equal(ci, M.ci)):
            self.fail(f"{tid}: export_csr structure differs from the model", where)
        if not same(v, M.vals, kind):
            bad = np.flatnonzero(~((v == M.vals) | (np.isnan(v) & np.isnan(M.vals))))
            self.fail(f"{tid}: export_csr values differ from the model ({kind}); first entries {bad[:5].tolist()}: got {v[bad[:5]].tolist()}, "
                      f"want {M.vals[bad[:5]].tolist()}", where)
        if kind == "minmax":
            self.m.adopt(tid, v)

    def check_plan(self, pid, where="step"):
        P, M = self.p[pid], self.m.p[pid]
        kind = "minmax" if M.c_semiring in sm.MINMAX else "exact"
        try:
            rp, ci, v = P.export_csr()
        except self.pkg.PemError as e:
            self.gpu_error(e)
            self.fail(f"{pid}: the model holds a current C, export_csr raised {e}", where)
        mrp, mci, mv = M.C
        if not (np.array_equal(rp, mrp) and np.array_equal(ci, mci)):
            self.fail(f"{pid}: C's structure differs from the model (nnz {len(ci)} / {len(mci)})", where)
        if not same(v, mv, kind):
            bad = np.flatnonzero(~((v == mv) | (np.isnan(v) & np.isnan(mv))))
            self.fail(f"{pid}: C's values differ from the model ({kind}); first entries {bad[:5].tolist()}: got {v[bad[:5]].tolist()}, "
                      f"want {mv[bad[:5]].tolist()}", where)
        if kind == "minmax":
            M.C = (mrp, mci, v.copy())

    def gpu_error(self, e):
        if getattr(e, "status", 0) == PEM_E_HIP:
            raise SeqGpuError(f"seed {self.seed}, step {self.step}: {e}\n{sg.dumps(self.prog[:self.step + 1])}") from e

    # ---- the audit ----------------------------------------------------------------------------------------------------------------
    def _rebuild(self, M, vals):
        return self.pkg.Tiled.from_csr(self.ctx, M.rows, M.cols, M.rp, M.ci, vals, dtype=M.dtype)

    def _dense_rows(self, n, dtype):
        """a dense 8 x n tiling of special-laden values: the A operand that makes a tiling's vals_t the B side of a plan"""
        key = (n, np.dtype(dtype).name)
        if key not in self.dense_a:
            ii, jj = np.meshgrid(np.arange(8, dtype=np.int32), np.arange(n, dtype=np.int32), indexing="ij")
            self.dense_a[key] = self.pkg.Tiled.from_coo(self.ctx, 8, n, ii.ravel(), jj.ravel(), sm.values(8 * n, 7, True, dtype), dtype=dtype)
        return self.dense_a[key]

    def audit_tiling(self, tid, where):
        """every info field and every pem_tiled_array against a from_csr rebuild from the model, and vals_t through both of its
        readers: as the B operand of a small dense-row plan, and mxv(transpose=True); trsv_info of every triangle whose schedule the
        model has as built, and ilu0_info of a factor"""
        T, M = self.t[tid], self.m.t[tid]
        self.check_tiling(tid, "exact", where)
        W = self._rebuild(M, M.vals)
        Wt = W if M.vals_t is M.vals else self._rebuild(M, M.vals_t)
        try:
            for f in INFO:
                if getattr(T, f) != getattr(W, f):
                    self.fail(f"{tid}: info field {f}: {getattr(T, f)}, a rebuild from the model has {getattr(W, f)}", where)
            for a in ARRAYS:
                x, y = T.array(a), W.array(a)
                if not (same(x, y) if a == "vals" else np.array_equal(x, y)):
                    self.fail(f"{tid}: array {a} differs from a from_csr rebuild of the model", where)
            A0 = self._dense_rows(M.rows, M.dtype)
            got, want = self.pkg.CPlan(self.ctx, A0, T), self.pkg.CPlan(self.ctx, A0, Wt)
            try:
                got.spgemm()
                want.spgemm()
                for x, y in zip(got.export_csr(), want.export_csr()):
                    if not same(x, y):
                        self.fail(f"{tid}: vals_t as the B operand of a plan differs from a rebuild of the model", where)
            finally:
                got.close()
                want.close()
            xv = self.dev(sm.values(M.rows, 8, True, M.dtype))
            self.uploaded()
            yt, wt = self.host(T.mxv(xv, transpose=True)), self.host(Wt.mxv(xv, transpose=True))
            if not same(yt, wt):
                self.fail(f"{tid}: vals_t under the column walk (mxv transpose) differs from a rebuild of the model", where)
            for uplo in ("lower", "upper"):      # only the triangles the model has as built: trsv_info would build the other
                if "trsv_" + uplo in M.built:
                    got, want = self._fields(T.trsv_info(uplo), TRSV_FIELDS), sm.trsv_fields(M, uplo)
                    if not np.array_equal(got, want):
                        self.fail(f"{tid}: trsv_info({uplo}) {dict(zip(TRSV_FIELDS, got.tolist()))}, trsvref's levels of the model's pattern "
                                  f"give {want.tolist()}", where)
            if M.prov is not None and M.prov[0] == "ilu0":
                got, want = self._fields(T.ilu0_info(), PIVOT_FIELDS), sm.pivot_fields(M)
                if not np.array_equal(got, want):
                    self.fail(f"{tid}: ilu0_info {dict(zip(PIVOT_FIELDS, got.tolist()))}, the model's factor gives {want.tolist()}", where)
        finally:
            if Wt is not W:
                Wt.close()
            W.close()

    def audit_plan(self, pid, where):
        P, M = self.p[pid], self.m.p[pid]
        info = P.info()
        want = dict(tile_row_begin=M.lo, tile_row_end=M.hi, row_begin=M.row0, row_end=M.row1)
        for k, v in want.items():
            if info[k] != v:
                self.fail(f"{pid}: info {k} = {info[k]}, the model has {v}", where)
        if M.state == 3 and info["nnz_c"] != len(M.C[1]):
            self.fail(f"{pid}: info nnz_c = {info['nnz_c']}, the model's C has {len(M.C[1])} entries", where)
        if P.semiring != M.semiring:
            self.fail(f"{pid}: semiring {P.semiring}, the model has {M.semiring}", where)
        for name, v in M.options.items():
            if P.get_option(name) != v:
                self.fail(f"{pid}: option {name} = {P.get_option(name)}, the model has {v}", where)
        if self.m.current(M):
            self.check_plan(pid, where)
        else:
            try:
                P.export_csr()
            except self.pkg.PemError as e:
                self.gpu_error(e)
                if e.status != sm.PEM_E_STATE:
                    self.fail(f"{pid}: export of a plan that is not current raised {e}, not PEM_E_STATE", where)
            else:
                self.fail(f"{pid}: the model says C is not current (state {M.state}), export_csr succeeded", where)
        if M.state >= 2:   # the symbolic arrays stay readable, and unchanged while no option changes
            try:
                arrays = {a: P.array(a) for a in SYMBOLIC}
            except self.pkg.PemError as e:
                self.gpu_error(e)
                self.fail(f"{pid}: the model has the plan at step {M.state}, reading its symbolic arrays raised {e}", where)
            old = self.snap.get(pid)
            if old is not None and old[0] == M.option_epoch:
                for a in SYMBOLIC:
                    if not np.array_equal(arrays[a], old[1][a]):
                        self.fail(f"{pid}: symbolic array {a} changed since the last audit with no option change", where)
            self.snap[pid] = (M.option_epoch, arrays)

    def audit_hierarchy(self, hid, where):
        """the info fields (bytes: not negative, nothing more) and every level's A_l, P_l, R_l by export_csr against the model"""
        H, M = self.h[hid], self.m.h[hid]
        info = H.info
        got, want = self._amg_fields(info), self.m.amg_fields(M)
        if not np.array_equal(got, want):
            self.fail(f"{hid}: info fields {got.tolist()}, the model has {want.tolist()}", where)
        if info["bytes"] < 0:
            self.fail(f"{hid}: info bytes = {info['bytes']}", where)
        for l, L in enumerate(self.m.levels(M)):
            for name, T in zip("APR", H.level(l)):
                if (T is None) != (L[name] is None):
                    self.fail(f"{hid}: level {l}: {name} is {'missing' if T is None else 'there'}, the model disagrees", where)
                if T is None:
                    continue
                rows, cols, mrp, mci, mv = L[name]
                rp, ci, v = T.export_csr()
                if (T.rows, T.cols) != (rows, cols) or not (np.array_equal(rp, mrp) and np.array_equal(ci, mci)):
                    self.fail(f"{hid}: level {l}: the structure of {name} differs from the model", where)
                if not same(v, mv):
                    self.fail(f"{hid}: level {l}: the values of {name} differ from the model", where)

    def audit(self, tids=None, pids=None, where="audit", hids=None):
        self.audits += 1
        for tid in (self.m.t if tids is None else tids):
            self.audit_tiling(tid, where)
        for pid in (self.m.p if pids is None else pids):
            self.audit_plan(pid, where)
        for hid in (self.m.h if hids is None else hids):
            self.audit_hierarchy(hid, where)
        self.keep.clear()

    # ---- the operations on the device: each returns what the call handed back (or None) ------------------------------------------------
    def g_from_coo(self, ids, a):
        rows, cols, I, J, V = sm.matrix(a["src"])
        self.t[a["out"]] = self.pkg.Tiled.from_coo(self.ctx, rows, cols, I, J, V, a["transpose"], dtype=sm.dt(a["dtype"]))

    def g_from_csr(self, ids, a):
        rows, cols, I, J, V = sm.matrix(a["src"])
        rp, ci, v = coo_to_csr(rows, cols, I, J, V)
        self.t[a["out"]] = self.pkg.Tiled.from_csr(self.ctx, rows, cols, rp, ci, v, dtype=sm.dt(a["dtype"]))

    def g_from_coo_device(self, ids, a):
        rows, cols, I, J, V = sm.matrix(a["src"])
        dtype = sm.dt(a["dtype"])
        dI, dJ, dV = self.dev(np.asarray(I, np.int32)), self.dev(np.asarray(J, np.int32)), self.dev(np.asarray(V, dtype))
        self.uploaded()
        self.t[a["out"]] = self.pkg.Tiled.from_coo_device(self.ctx, rows, cols, len(I), dI.data_ptr(), dJ.data_ptr(), dV.data_ptr(), a["transpose"],
                                                          dtype=dtype)

    def g_close(self, ids, a):
        self.t.pop(ids[0]).close()

    def g_save_load(self, ids, a):
        path = f"{self.tmpdir}/{a['out']}.pemt"
        self.t[ids[0]].save(path)
        self.t[a["out"]] = self.pkg.Tiled.load(self.ctx, path)

    def g_plan_create(self, ids, a):
        A, B = self.t[ids[0]], self.t[ids[1]]
        M = self.t[ids[2]] if ids[2] is not None else None
        self.p[a["out"]] = self.pkg.CPlan(self.ctx, A, B, a["lo"], a["hi"], mask=M, complement=a["complement"], semiring=a["semiring"])

    def g_plan_close(self, ids, a):
        self.p.pop(ids[0]).close()
        self.snap.pop(ids[0], None)

    def g_step1(self, ids, a):
        self.p[ids[0]].step1()

    def g_step2(self, ids, a):
        self.p[ids[0]].step2()

    def g_step3(self, ids, a):
        self.p[ids[0]].step3()

    def g_spgemm(self, ids, a):
        self.p[ids[0]].spgemm()

    def g_set_semiring(self, ids, a):
        self.p[ids[0]].set_semiring(a["semiring"])

    def g_set_option(self, ids, a):
        self.p[ids[0]].set_option(a["name"], a["value"])

    def g_export_csr(self, ids, a):
        return self.p[ids[0]].export_csr()

    def g_export_coo(self, ids, a):
        return self.p[ids[0]].export_coo()

    def g_from_cplan(self, ids, a):
        self.t[a["out"]] = self.pkg.Tiled.from_cplan(self.p[ids[0]], a["transpose"])

    def g_set_values_from_cplan(self, ids, a):
        self.t[ids[0]].set_values_from_cplan(self.p[ids[1]])

    def g_ewise(self, ids, a):
        self.t[a["out"]] = self.pkg.Tiled.ewise(self.t[ids[0]], self.t[ids[1]], a["op"], a["pattern"], a["alpha"], a["beta"])

    def g_set_values_from_ewise(self, ids, a):
        self.t[ids[0]].set_values_from_ewise(self.t[ids[1]], self.t[ids[2]])

    def g_select(self, ids, a):
        self.t[a["out"]] = self.t[ids[0]].select(a["op"], a["thunk"])

    def g_set_values_from_select(self, ids, a):
        self.t[ids[0]].set_values_from_select(self.t[ids[1]])

    def _sddmm_dev(self, M, a, dtype):
        k = a["k"]
        Xw, Yw, _, _ = self.m.sddmm_operands(M, a, dtype)
        X, Y = self.dev(Xw)[:, 2:2 + k], self.dev(Yw)[:, 5:5 + k]
        self.uploaded()
        return X, Y

    def g_sddmm(self, ids, a):
        X, Y = self._sddmm_dev(self.m.t[ids[0]], a, sm.dt(a["dtype"]))
        self.t[a["out"]] = self.t[ids[0]].sddmm(X, Y, a["semiring"])

    def g_set_values(self, ids, a):
        M = self.m.t[ids[0]]
        self.t[ids[0]].set_values(sm.values(M.nnz, a["seed"], a["special"], M.dtype), a["order"])

    def g_set_values_device(self, ids, a):
        M = self.m.t[ids[0]]
        dV = self.dev(sm.values(M.nnz, a["seed"], a["special"], M.dtype))
        self.uploaded()
        self.t[ids[0]].set_values_device(dV, a["order"])

    def g_set_values_sddmm(self, ids, a):
        M = self.m.t[ids[0]]
        X, Y = self._sddmm_dev(M, a, M.dtype)
        self.t[ids[0]].set_values_sddmm(X, Y, a["semiring"], accumulate=a["accumulate"])

    def g_mxv(self, ids, a):
        M = self.m.t[ids[0]]
        nx, ny = (M.rows, M.cols) if a["transpose"] else (M.cols, M.rows)
        x = self.dev(sm.values(nx, a["seed"], a["special"], M.dtype))
        y = self.dev(sm.values(ny, a["seed"] + 1, a["special"], M.dtype)) if a["accumulate"] else None
        self.uploaded()
        return self.host(self.t[ids[0]].mxv(x, a["semiring"], a["transpose"], out=y, accumulate=a["accumulate"]))

    def g_reduce(self, ids, a):
        M = self.m.t[ids[0]]
        ny = M.cols if a["dim"] == "cols" else M.rows
        y = self.dev(sm.values(ny, a["seed"] + 1, a["special"], M.dtype)) if a["accumulate"] else None
        self.uploaded()
        return self.host(self.t[ids[0]].reduce(a["op"], a["dim"], out=y, accumulate=a["accumulate"]))

    def g_spmm(self, ids, a):
        M = self.m.t[ids[0]]
        k = a["k"]
        Xw, Yfull = self.m.spmm_operands(M, a)
        X, Y = self.dev(Xw), self.dev(Yfull)
        self.uploaded()
        self.t[ids[0]].spmm(X[:, 1:1 + k], a["semiring"], a["transpose"], out=Y[:, :k], accumulate=a["accumulate"])
        return self.host(Y)

    # ---- the second operation set --------------------------------------------------------------------------------------------------
    def g_apply(self, ids, a):
        self.t[a["out"]] = self.t[ids[0]].apply(a["op"], a["thunk"])

    def g_set_values_from_apply(self, ids, a):
        self.t[ids[0]].set_values_from_apply(self.t[ids[1]])

    def g_transpose(self, ids, a):
        self.t[a["out"]] = self.t[ids[0]].transpose()

    def g_set_values_from_transpose(self, ids, a):
        self.t[ids[0]].set_values_from_transpose(self.t[ids[1]])

    def _index_arg(self, spec):
        """an index list of a record as extract takes it: None, a slice, a host array or a device tensor"""
        if spec is None:
            return None
        if spec[0] == "slice":
            return slice(*spec[1:])
        L = np.asarray(spec[1], np.int32)
        return self.dev(L) if spec[0] == "device" else L

    def g_extract(self, ids, a):
        rows, cols = self._index_arg(a["rows"]), self._index_arg(a["cols"])
        self.uploaded()
        self.t[a["out"]] = self.t[ids[0]].extract(rows, cols)

    def g_set_values_from_extract(self, ids, a):
        self.t[ids[0]].set_values_from_extract(self.t[ids[1]])

    def g_kron(self, ids, a):
        self.t[a["out"]] = self.pkg.Tiled.kron(self.t[ids[0]], self.t[ids[1]], a["op"])

    def g_set_values_from_kron(self, ids, a):
        self.t[ids[0]].set_values_from_kron(self.t[ids[1]], self.t[ids[2]])

    def g_concat(self, ids, a):
        cells = [None if h is None else self.t[h] for h in ids]
        gc = a["grid"][1]
        self.t[a["out"]] = self.pkg.Tiled.concat([cells[k:k + gc] for k in range(0, len(cells), gc)], a["row_sizes"], a["col_sizes"])

    def g_set_values_from_concat(self, ids, a):
        self.t[ids[0]].set_values_from_concat([[None if h is None else self.t[h] for h in ids[1:]]])

    def g_ilu0(self, ids, a):
        self.t[a["out"]] = self.t[ids[0]].ilu0()

    def g_set_values_from_ilu0(self, ids, a):
        self.t[ids[0]].set_values_from_ilu0(self.t[ids[1]])

    def g_trsv(self, ids, a):
        M = self.m.t[ids[0]]
        b = sm.values(M.rows, a["seed"], a["special"], M.dtype)
        if a.get("overlap"):             # b and out one element apart in one buffer
            buf = self.dev(np.concatenate([b, b[:1]]))
            db, out = buf[:M.rows], buf[1:]
        else:
            db = self.dev(b)
            out = db if a["in_place"] else self.dev(sm.values(M.rows, a["seed"] + 1, True, M.dtype))
        self.uploaded()
        return self.host(self.t[ids[0]].trsv(db, a["uplo"], a["unit_diag"], out=out))

    def g_lu_solve(self, ids, a):
        M = self.m.t[ids[0]]
        db = self.dev(sm.values(M.rows, a["seed"], a["special"], M.dtype))
        self.uploaded()
        return self.host(self.t[ids[0]].lu_solve(db))

    def _scale_vectors(self, M, a):
        r, c = (None if a[k] is None else self.dev(sm.values(n, a[k], a["special"], M.dtype)) for k, n in (("rows", M.rows), ("cols", M.cols)))
        self.uploaded()
        return r, c

    def g_scale(self, ids, a):
        r, c = self._scale_vectors(self.m.t[ids[0]], a)
        self.t[a["out"]] = self.t[ids[0]].scale(r, c, a["op"])

    def g_set_values_from_scale(self, ids, a):
        r, c = self._scale_vectors(self.m.t[ids[0]], a)      # (a scale keeps the shape: the vectors fit whatever source is named)
        self.t[ids[0]].set_values_from_scale(self.t[ids[1]], r, c)

    def g_assign(self, ids, a):
        rows, cols = self._index_arg(a["rows"]), self._index_arg(a["cols"])
        self.uploaded()
        self.t[a["out"]] = self.t[ids[0]].assign(self.t[ids[1]], rows, cols, a["accum"])

    def g_set_values_from_assign(self, ids, a):
        self.t[ids[0]].set_values_from_assign(self.t[ids[1]], self.t[ids[2]])

    def g_build(self, ids, a):
        dtype = sm.dt(a["dtype"])
        rows, cols, I, J, V = sm.triplets(a, dtype)
        self.t[a["out"]] = self.pkg.Tiled.build(self.ctx, rows, cols, I, J, V, a["dup"], a["transpose"], dtype=dtype, keep_map=a["keep_map"])

    def g_build_device(self, ids, a):
        dtype = sm.dt(a["dtype"])
        rows, cols, I, J, V = sm.triplets(a, dtype)
        dI, dJ, dV = self.dev(np.asarray(I, np.int32)), self.dev(np.asarray(J, np.int32)), self.dev(V)
        self.uploaded()
        self.t[a["out"]] = self.pkg.Tiled.build_device(self.ctx, rows, cols, len(I), dI.data_ptr(), dJ.data_ptr(), dV.data_ptr(), a["dup"],
                                                       a["transpose"], dtype=dtype, keep_map=a["keep_map"])

    def g_set_values_from_build(self, ids, a):
        dV = self.dev(sm.values(a["nnz_in"], a["seed"], a["special"], self.m.t[ids[0]].dtype))
        self.uploaded()
        self.t[ids[0]].set_values_from_build(dV)

    def g_sampled_mxm(self, ids, a):
        self.t[a["out"]] = self.t[ids[0]].sampled_mxm(self.t[ids[1]], self.t[ids[2]], a["semiring"], a["transpose_b"])

    def g_set_values_sampled_mxm(self, ids, a):
        self.t[ids[0]].set_values_sampled_mxm(self.t[ids[1]], self.t[ids[2]], a["semiring"], a["transpose_b"], a["accumulate"])

    def g_triangle_count(self, ids, a):
        return np.array([self.pkg.triangle_count(self.t[ids[0]])], np.int64)

    def g_select_topk(self, ids, a):
        self.t[a["out"]] = self.t[ids[0]].select_topk(a["k"], a["order"], a["dim"])

    def _frontier_dev(self, M, a, index=False):
        """the operands of a frontier or arg record on the device; every output vector is uploaded, so that what a call must not
        write still holds what was uploaded"""
        x, y0, idx0, present, mask = self.m.frontier_operands(M, a)
        ny = len(y0)
        d = dict(x=None if x is None else self.dev(x), y=self.dev(y0), idx=self.dev(idx0) if index else None,
                 present=None if present is None else self.dev(present), mask=None if mask is None else self.dev(mask),
                 out_present=self.dev(np.full(ny, 7, np.uint8)) if a["out_present"] else None)
        self.uploaded()
        return d

    def g_mxv_frontier(self, ids, a):
        d = self._frontier_dev(self.m.t[ids[0]], a)
        y = self.t[ids[0]].mxv_frontier(d["x"], d["present"], d["mask"], a["mask"] == "complement", a["semiring"], a["transpose"], out=d["y"],
                                        accumulate=a["accumulate"], out_present=d["out_present"])
        return (self.host(y), self.host(d["out_present"])) if a["out_present"] else self.host(y)

    def g_mxv_arg(self, ids, a):
        d = self._frontier_dev(self.m.t[ids[0]], a, index=True)
        values = a["kind"] in argref.VALUE_KINDS
        y, idx = self.t[ids[0]].mxv_arg(d["x"], a["kind"], a["transpose"], d["present"], d["mask"], a["mask"] == "complement",
                                        out=d["y"] if values else None, out_index=d["idx"], out_present=d["out_present"], accumulate=a["accumulate"])
        return ((self.host(y),) if values else ()) + (self.host(idx),) + ((self.host(d["out_present"]),) if a["out_present"] else ())

    def g_reduce_arg(self, ids, a):
        y, idx = self.t[ids[0]].reduce_arg(a["op"], a["dim"])
        return self.host(y), self.host(idx)

    def g_bfs(self, ids, a):
        levels, depth, reached = self.t[ids[0]].bfs(a["source"], a["transpose"])
        return self.host(levels), np.array([depth, reached], np.int64)

    def g_bfs_parents(self, ids, a):
        levels, parents, depth, reached = self.t[ids[0]].bfs_parents(a["source"], a["transpose"])
        return self.host(levels), self.host(parents), np.array([depth, reached], np.int64)

    @staticmethod
    def _fields(info, names):
        return np.array([info[k] for k in names], np.int64)

    def g_trsv_info(self, ids, a):
        return self._fields(self.t[ids[0]].trsv_info(a["uplo"]), TRSV_FIELDS)

    def g_ilu0_info(self, ids, a):
        return self._fields(self.t[ids[0]].ilu0_info(), PIVOT_FIELDS)

    # ---- the third operation set: graph routines -------------------------------------------------------------------------------------
    def _graph_call(self, kind, tid, n, symmetric, fn):
        """fn() under the allocation rule of the graph scratch: a call whose demand does not exceed the largest any graph call has
        made on this context allocates nothing (where it does not build the column schedule either).  The demand is tracked per
        context for its whole life: Context.trim returns wholly free slabs only, and the scratch is a block in use, so it survives a
        trim.  The hierarchies' own aggregate calls are not counted: the bound stays a lower one."""
        demand, known = sm.graph_demand(kind, n), getattr(self.ctx, "_seq_graph_demand", 0)
        quiet = tid in self.pre_built and demand <= known and (symmetric or "mx_cols" in self.pre_built[tid])
        before = self.ctx.memory_stats()
        out = fn()
        after = self.ctx.memory_stats()
        if quiet and any(after[k] != before[k] for k in ("block_allocs", "driver_allocs")):
            self.fail(f"{kind} with a scratch demand of {demand} bytes allocated ({before} -> {after}); the context had served {known}")
        self.ctx._seq_graph_demand = max(known, demand)
        return out

    def _prio_dev(self, n, a):
        """seed / priority of a graph call: a seed, a host array or a device tensor"""
        spec = a["prio"]
        if spec[0] == "seed":
            return dict(seed=spec[1])
        arr = sm.priority(n, spec)
        return dict(priority=self.dev(arr.view(np.int32)) if spec[1] == "device" else arr)

    def _poison(self, n, dtype=np.int32, value=POISON_I):
        return self.dev(np.full(n, value, dtype))

    def g_colour(self, ids, a):
        T, n = self.t[ids[0]], self.m.t[ids[0]].rows
        kw = self._prio_dev(n, a)
        out = kw["priority"] if a.get("overlap") else self._poison(n)
        self.uploaded()
        c, nc, rounds = self._graph_call("colour", ids[0], n, a["symmetric"], lambda: T.colour(symmetric=a["symmetric"], out=out, **kw))
        return self.host(c), np.array([nc, rounds], np.int64)

    def g_components(self, ids, a):
        T, n = self.t[ids[0]], self.m.t[ids[0]].rows
        out, out_ids = self._poison(n), self._poison(n) if a["ids"] else None
        self.uploaded()
        labels, cid, nc, rounds = self._graph_call("components", ids[0], n, a["symmetric"],
                                                   lambda: T.components(symmetric=a["symmetric"], out=out, ids=a["ids"], out_ids=out_ids))
        return (self.host(labels),) + ((self.host(cid),) if a["ids"] else ()) + (np.array([nc, rounds], np.int64),)

    def g_colour_order(self, ids, a):
        T, n = self.t[ids[0]], self.m.t[ids[0]].rows
        out = self._poison(n)
        if a["of"] == "colour":
            kw = self._prio_dev(n, a)
            self.uploaded()
            keys, nk, _ = self._graph_call("colour", ids[0], n, a["symmetric"], lambda: T.colour(symmetric=a["symmetric"], out=out, **kw))
        else:
            labels = self._poison(n)
            self.uploaded()
            _, keys, nk, _ = self._graph_call("components", ids[0], n, a["symmetric"],
                                              lambda: T.components(symmetric=a["symmetric"], out=labels, out_ids=out))
        self.pre_built.get(ids[0], set()).add("mx_cols")    # (the first call built the schedule, if any had to)
        perm, offsets = self._graph_call("colour_order", ids[0], n, True, lambda: self.pkg.colour_order(self.ctx, keys, nk))
        return self.host(keys), self.host(perm), self.host(offsets), np.array([nk], np.int64)

    def g_mis(self, ids, a):
        T, n = self.t[ids[0]], self.m.t[ids[0]].rows
        out = self._poison(n, np.uint8, POISON_B)
        kw = self._prio_dev(n, a)
        self.uploaded()
        if a["distance"] not in (1, 2):          # (Tiled.mis refuses it itself: the library's own refusal is asked for)
            count, rounds = C.c_int64(), C.c_int32()
            self.pkg._check(self.pkg.lib().pem_tiled_mis(self.ctx._h, T._h, int(a["distance"]), int(a["symmetric"]), kw.get("seed", 0), None,
                                                         C.c_void_p(out.data_ptr()), C.byref(count), C.byref(rounds)))
            return None
        s, count, rounds = self._graph_call("mis", ids[0], n, a["symmetric"], lambda: T.mis(a["distance"], symmetric=a["symmetric"], out=out, **kw))
        return self.host(s), np.array([count, rounds], np.int64)

    def g_aggregate(self, ids, a):
        T, n = self.t[ids[0]], self.m.t[ids[0]].rows
        out = self._poison(n)
        kw = self._prio_dev(n, a)
        self.uploaded()
        agg, roots, nc, rounds = self._graph_call("aggregate", ids[0], n, a["symmetric"],
                                                  lambda: T.aggregate(symmetric=a["symmetric"], out=out, roots=a["roots"], **kw))
        return (self.host(agg),) + ((self.host(roots),) if a["roots"] else ()) + (np.array([nc, rounds], np.int64),)

    # ---- the third operation set: solvers --------------------------------------------------------------------------------------------
    def g_krylov_create(self, ids, a):
        A, pc, pre = self.t[ids[0]], a["precond"], ids[1]
        if (pc == "lu") != (pre in self.t):      # (the Krylov class cannot say it: lu without a factor, a factor under none / diag)
            opts = self.pkg.KrylovOpts(self.pkg.KRYLOV_METHODS.index(a["method"]), ("none", "diag", "lu").index(pc), a["max_iters"],
                                       a["check_every"], a["rtol"], a["atol"])
            h = C.c_void_p()
            self.pkg._check(self.pkg.lib().pem_krylov_create(self.ctx._h, A._h, C.byref(opts), self.t[pre]._h if pre in self.t else None, C.byref(h)))
            self.fail("pem_krylov_create accepted a call the header refuses")
        precond = {"none": None, "diag": "diag"}[pc] if pc in ("none", "diag") else self.t[pre] if pc == "lu" else self.h[pre]
        self.k[a["out"]] = self.pkg.Krylov(A, a["method"], precond, a["max_iters"], a["check_every"], a["rtol"], a["atol"])

    def g_krylov_close(self, ids, a):
        self.k.pop(ids[0]).close()

    def _solve_dev(self, M, a, max_iters, diag):
        b, x0, minv = self.m.solve_operands(M.rows, a, M.dtype)
        d = dict(b=self.dev(b), x=self.dev(x0) if a["x0"] else None, minv=self.dev(minv) if diag else None,
                 hist=self.dev(np.full(max_iters + 1, POISON_F)) if a["history"] else False)
        self.uploaded()
        return d

    def _solved(self, a, x, info, hist, launches):
        """what a solve handed back, in the model's order; the part of the history past iters still holds what it held"""
        if launches is not None and info["launches"] != launches:
            self.fail(f"launches = {info['launches']}, the header's formula gives {launches}")
        out = (self.host(x), np.array([info["iters"], info["status_code"], info["readbacks"]], np.int64),
               np.array([info["bb"], info["rr"], info["threshold"]], np.float64))
        if a["history"]:
            h = self.host(hist)
            if not np.all(h[info["iters"] + 1:] == POISON_F):
                self.fail(f"the history was written past entry iters = {info['iters']}")
            out += (h[:info["iters"] + 1],)
        return out

    def _launches(self, e, T):
        return krylovref.launches(e["method"], "lu" if e["precond"] in ("lu", "amg") else e["precond"], e["stop_iter"], e["check_every"], e["max_iters"], T)

    def g_krylov_solve(self, ids, a):
        K, MK = self.k[ids[0]], self.m.k[ids[0]]
        M = self.m.t[MK.a]
        d = self._solve_dev(M, a, MK.max_iters, MK.precond == "diag")
        if a.get("wrong_form"):                  # the fp64 entry point on an fp32 solver
            res = self.pkg.KrylovResult()
            self.pkg._check(self.pkg.lib().pem_krylov_solve(self.ctx._h, K._h, C.c_void_p(d["b"].data_ptr()), C.c_void_p(d["x"].data_ptr()) if a["x0"] else
                                                            C.c_void_p(d["b"].data_ptr()), None, None, C.byref(res)))
            return None
        x, info = K.solve(d["b"], x=d["x"], minv=d["minv"], history=d["hist"])
        T = 0
        if MK.precond == "lu":
            F = self.t[MK.pre]
            T = F.trsv_info("lower")["launches"] + F.trsv_info("upper")["launches"]
        elif MK.precond == "amg":
            T = int(self.m.amg_fields(self.m.h[MK.pre])[1])
        return self._solved(a, x, info, d["hist"], self._launches(self.res.extra, T))

    def g_tiled_solve(self, ids, a):
        M = self.m.t[ids[0]]
        d = self._solve_dev(M, a, a["max_iters"], False)
        x, info = self.t[ids[0]].solve(d["b"], a["method"], None if a["precond"] == "none" else a["precond"], x=d["x"], max_iters=a["max_iters"],
                                       check_every=a["check_every"], rtol=a["rtol"], atol=a["atol"], history=d["hist"])
        # (the launches of its own factor's solves are not to be had: the formula is checked without a preconditioner only)
        return self._solved(a, x, info, d["hist"], self._launches(self.res.extra, 0) if a["precond"] == "none" else None)

    # ---- the third operation set: hierarchies ------------------------------------------------------------------------------------------
    def g_amg_create(self, ids, a):
        self.h[a["out"]] = self.pkg.Amg(self.t[ids[0]], smooth=bool(a["smooth"]), symmetric=a["symmetric"], seed=0, max_levels=16,
                                        coarse_size=a["coarse_size"], sweeps=a["sweeps"], coarse_sweeps=a["coarse_sweeps"], omega=sm.AMG_OMEGA,
                                        refreshable=bool(a["refreshable"]))

    def g_amg_refresh(self, ids, a):
        self.h[ids[0]].refresh()

    def g_amg_apply(self, ids, a):
        M = self.m.t[self.m.h[ids[0]].a]
        r, out = self.dev(sm.values(M.rows, a["seed"], a["special"], M.dtype)), self._poison(M.rows, M.dtype, POISON_F)
        self.uploaded()
        return self.host(self.h[ids[0]].apply(r, out=out))

    @staticmethod
    def _amg_fields(i):
        return np.array([i["levels"], i["launches"]] + i["rows"] + i["nnz"] + i["p_nnz"] + i["aggregate_rounds"], np.int64)

    def g_amg_info(self, ids, a):
        info = self.h[ids[0]].info
        if info["bytes"] < 0:
            self.fail(f"info bytes = {info['bytes']}")
        return self._amg_fields(info)

    def g_amg_level(self, ids, a):
        """the borrowed handle goes to the reader under a name of its own, next to the model's copy of that level"""
        H = self.m.h[ids[0]]
        T = self.h[ids[0]].level(a["level"])["APR".index(a["which"])]
        op, args = a["reader"]
        if op == "export_csr":
            return T.export_csr()
        self.t["~level"], self.m.t["~level"] = T, self.m.level_tiling(H, a["level"], a["which"])
        try:
            return getattr(self, "g_" + op)(("~level",), args)
        finally:
            del self.t["~level"], self.m.t["~level"]

    def g_amg_close(self, ids, a):
        self.h.pop(ids[0]).close()

    def g_trim(self, ids, a):
        self.ctx.trim()

    def g_reserve(self, ids, a):
        self.ctx.reserve(a["bytes"])

    def g_synchronize(self, ids, a):
        self.ctx.synchronize()

    # ---- one step, one program ---------------------------------------------------------------------------------------------------
    def run_step(self, i, rec):
        self.step, self.rec = i, rec
        op, ids, a = rec
        named_t = [h for h in ids if h in self.m.t]
        named_p = [h for h in ids if h in self.m.p]
        named_h = [h for h in ids if h in self.m.h]
        self.pre_built = {h: set(self.m.t[h].built) for h in named_t}
        res = self.res = self.m.apply(rec)
        if self.log:
            self.log(f"step {i}: {sg.dumps([rec])} -> model status {res.status}")
        try:
            got = getattr(self, "g_" + op)(ids, a)
        except self.pkg.PemError as e:
            self.gpu_error(e)
            if res.status == 0:
                self.fail(f"the model accepts the call, the library raised {e}")
            if e.status != res.status:
                self.fail(f"the model predicts status {res.status}, the library raised {e}")
            if "out" in a and (a["out"] in self.t or a["out"] in self.k or a["out"] in self.h):
                self.fail("a refused call left a handle behind")
            self.audit(named_t, named_p, where="after the refusal", hids=named_h)   # a refused call leaves every handle it named as it was
            return
        if res.status != 0:
            self.fail(f"the model predicts status {res.status}, the library accepted the call")
        if res.wrote in self.m.t:
            self.check_tiling(res.wrote, res.kind)
        elif res.wrote in self.m.p:
            self.check_plan(res.wrote)
        if res.out is not None:
            want = res.out if isinstance(res.out, tuple) else (res.out,)
            got = got if isinstance(got, tuple) else (got,)
            if len(got) != len(want):
                self.fail(f"the call handed back {len(got)} results, the model has {len(want)}")
            for n, (x, y) in enumerate(zip(got, want)):
                ok = same(x, y, res.kind) if np.asarray(y).dtype.kind == "f" else np.array_equal(x, y)
                if not ok:
                    self.fail(f"result {n} of the call differs from the model ({res.kind})")
        self.keep.clear()

    def run(self, prog, seed=None):
        """the whole program; returns the number of steps run.  The pool is closed afterwards, also on a mismatch."""
        self.seed, self.prog = seed, list(prog)
        try:
            for i, rec in enumerate(self.prog):
                self.run_step(i, rec)
                if (i + 1) % AUDIT_EVERY == 0 or i + 1 == len(self.prog):
                    self.rec = None
                    self.audit()
        finally:
            self.close()
        return len(self.prog)
