"""Runner of the sequence test: executes a program of tests/seqgen.py step by step on the GPU and on the host model of
tests/seqmodel.py, and compares after every step (tests/test_gpu_seq.py drives it, tools/seq_replay.py replays one program).

After every step:
  - a refusal the model predicts must come back as PemError with exactly that status, and the handles the call named are audited;
  - a call the model accepts must succeed;
  - the handle the step wrote is compared in full: a tiling by export_csr() (structure exact, values by `same`: equal bits, NaN equals
    NaN, +0 equals -0 only under min / max), a plan whose C is current by export_csr() alike, a dense result element for element.
Every AUDIT_EVERY steps and at the end, every live handle is audited (audit_tiling, audit_plan): the damage this suite looks for is
to a handle the step did not name.  There is no tolerance anywhere and no entry is left out.

Where the header leaves bits open (the sign of a zero under min / max, NaN payloads) the model adopts the device's bits after the
comparison under that rule has passed, so that everything computed from them later is compared exactly again.

A mismatch raises SeqMismatch; its message carries the seed, the step, the failing record and the program up to that step in the
text form tools/seq_replay.py reads.  A HIP error status (PEM_E_HIP) raises SeqGpuError, after which nothing more is run.
"""
import numpy as np
import torch

import argref
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

    def audit(self, tids=None, pids=None, where="audit"):
        self.audits += 1
        for tid in (self.m.t if tids is None else tids):
            self.audit_tiling(tid, where)
        for pid in (self.m.p if pids is None else pids):
            self.audit_plan(pid, where)
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
        res = self.m.apply(rec)
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
            if "out" in a and a["out"] in self.t:
                self.fail("a refused call left a handle behind")
            self.audit(named_t, named_p, where="after the refusal")   # a refused call leaves every handle it named as it was
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
