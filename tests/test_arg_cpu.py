"""CPU: argref, the host model of the arg folds, proved against what the project already trusts -- its
values are frontierref's under the semiring of the same name, its index points at an entering term equal to the value and no lower
index does, the index kinds are min / max of the filtered row's indices, reduce_arg is mxv_arg with x = 0, and the levels of
bfs_parents are frontierref.bfs's with every parent the least vertex of the previous level with the edge.  Also: the header declares
the five symbols and the binding lists them."""
import os
import re

import numpy as np
import pytest

import argref as ar
import frontierref as fr
import mxvref as mr
from matgen import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = cases()
TIE = np.array([-1.0, -0.0, 0.0, 1.0, 2.0, np.inf, -np.inf, np.nan])
MINMAX = ar.VALUE_KINDS
NAMES = ("one_entry", "ragged_37", "dense_tile", "rect_33x65_AAt", "empty_rows", "empty_matrix", "powerlaw_600")


def _same(got, want, kind="plus_times"):
    """the rule of test_gpu_frontier.py: equal bits, NaN for NaN, and under min / max any zero for a zero"""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    ok = (got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want))
    if kind in MINMAX:
        ok |= (got == 0) & (want == 0)
    return bool(np.all(ok))


def _ties(n, rng, dtype):
    """values drawn to tie: the eight specials, and a random one in eight"""
    v = rng.choice(TIE, n)
    r = rng.random(n) < 0.125
    v[r] = rng.standard_normal(int(r.sum()))
    return v.astype(dtype)


def _csr(name, rng, dtype):
    rows, cols, I, J, V, _ = CASES[name]
    I, J = np.asarray(I, np.int64), np.asarray(J, np.int64)
    o = np.lexsort((J, I))
    rp = np.zeros(rows + 1, np.int64)
    np.cumsum(np.bincount(I, minlength=rows), out=rp[1:])
    return rows, cols, rp, J[o], _ties(len(V), rng, dtype)


def _rows_of(rows, cols, rp, ci, v, tr):
    """(ny, rowptr, colidx, vals) of the oriented matrix"""
    if tr:
        rp, ci, v = mr.transpose_csr(rows, cols, rp, ci, v)
        rows, cols = cols, rows
    return rows, cols, rp, ci, v


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
@pytest.mark.parametrize("name", NAMES)
def test_model_against_the_frontier_model(name, dtype):
    rng = np.random.default_rng(len(name) + 17)
    rows, cols, rp, ci, v = _csr(name, rng, dtype)
    ties = 0
    for tr in (False, True):
        ny, nx, orp, oci, ov = _rows_of(rows, cols, rp, ci, v, tr)
        for present, mask, comp in ((None, None, False), (rng.random(nx) < 0.5, rng.random(ny) < 0.5, False),
                                    (rng.random(nx) < 0.1, rng.random(ny) < 0.5, True), (np.zeros(nx, bool), None, False)):
            x = _ties(nx, rng, dtype)
            if present is not None:
                x[~present] = np.nan
            y_old, idx_old = _ties(ny, rng, dtype), rng.integers(-2, nx + 1, ny).astype(np.int32)
            pres = np.ones(nx, bool) if present is None else present
            allowed = fr.allowed_of(ny, mask, comp)
            for acc in (False, True):
                for kind in ar.VALUE_KINDS:
                    y, idx, po = ar.mxv_arg(rows, cols, rp, ci, v, x, kind, dtype, present, mask, comp, y_old, idx_old, acc, tr)
                    wy, wpo = fr.mxv_frontier(rows, cols, rp, ci, v, x, kind, dtype, present, mask, comp, y_old, acc, None, tr)
                    assert _same(y, wy, kind), (name, kind, tr, acc)
                    assert np.array_equal(po, wpo)
                    for i in range(ny):
                        js = oci[orp[i]:orp[i + 1]]
                        keep = pres[js]
                        js, a = js[keep], np.asarray(ov[orp[i]:orp[i + 1]], dtype)[keep]
                        with np.errstate(all="ignore"):
                            t = a * x[js] if kind == "max_times" else a + x[js]
                        if not allowed[i]:
                            assert idx[i] == idx_old[i]
                            continue
                        old = y_old[i]
                        wins = ~np.isnan(t)
                        if acc and not np.isnan(old):
                            wins &= (t < old) if kind == "min_plus" else (t > old)
                        if not wins.any():
                            assert idx[i] == (idx_old[i] if acc else -1)
                            continue
                        k = int(np.flatnonzero(js == idx[i])[0])   # the index points at an entering term ...
                        assert t[k] == y[i] and wins[k]              # ... equal to the value, a winner ...
                        assert not np.any(t[:k] == y[i])             # ... and no lower index holds an equal one
                        ties += int(np.sum(t == y[i]) > 1)
                for kind in ar.INDEX_KINDS:
                    y, idx, po = ar.mxv_arg(rows, cols, rp, ci, v, None, kind, dtype, present, mask, comp, None, idx_old, acc, tr)
                    assert y is None
                    _, wpo = fr.mxv_frontier(rows, cols, rp, ci, v, None, "plus_pair", dtype, present, mask, comp, None, acc, None, tr)
                    assert np.array_equal(po, wpo)
                    f = min if kind == "min_index" else max
                    for i in range(ny):
                        js = oci[orp[i]:orp[i + 1]]
                        js = [int(j) for j in js[pres[js]]]
                        if not allowed[i]:
                            want = idx_old[i]
                        elif acc:
                            want = f(js + [int(idx_old[i])] * int(idx_old[i] >= 0)) if js else idx_old[i]
                        else:
                            want = f(js) if js else -1
                        assert idx[i] == want, (name, kind, tr, acc, i)
    if name in ("ragged_37", "dense_tile", "powerlaw_600"):
        assert ties > 10, "the values were drawn to tie and did not"


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
@pytest.mark.parametrize("name", NAMES)
def test_reduce_arg_is_mxv_arg_with_a_zero_x(name, dtype):
    rng = np.random.default_rng(len(name) + 5)
    rows, cols, rp, ci, v = _csr(name, rng, dtype)
    for dim in ("rows", "cols"):
        tr = dim == "cols"
        nx = rows if tr else cols
        for op, kind in (("min", "min_plus"), ("max", "max_plus")):
            y, idx = ar.reduce_arg(rows, cols, rp, ci, v, op, dtype, dim)
            wy, widx, _ = ar.mxv_arg(rows, cols, rp, ci, v, np.zeros(nx, dtype), kind, dtype, transpose=tr)
            assert _same(y, wy, kind) and np.array_equal(idx, widx), (name, dim, op)
            assert _same(y, mr.reduce(rows, cols, rp, ci, v, op, dtype, dim=dim), kind)


@pytest.mark.parametrize("name", ("powerlaw_600", "banded_500_AAt", "empty_rows", "diag_100", "rand_300"))
def test_bfs_parents_model(name):
    rng = np.random.default_rng(3)
    n, _, rp, ci, _ = _csr(name, rng, np.float64)
    several = 0
    for tr in (False, True):
        for src in (0, n // 2, n - 1):
            level, parent, depth, reached = ar.bfs_parents(n, rp, ci, src, tr)
            wl, wd, wr = fr.bfs(n, rp, ci, src, tr)
            assert np.array_equal(level, wl) and (depth, reached) == (wd, wr)
            _, _, orp, oci, _ = _rows_of(n, n, rp, ci, np.zeros(len(ci)), tr)
            assert parent[src] == src
            count = ar.candidate_parents(n, rp, ci, level, tr)
            for w in range(n):
                if w == src:
                    continue
                cands = [u for u in range(n) if level[u] >= 0 and level[u] + 1 == level[w] and w in oci[orp[u]:orp[u + 1]]]
                assert parent[w] == (min(cands) if level[w] > 0 else -1)
                assert count[w] == len(cands)
                several += len(cands) > 1
    if name in ("powerlaw_600", "banded_500_AAt", "rand_300"):
        assert several > 0


def test_header_and_binding_name_the_symbols(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pem_spgemm.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pem_[a-z0-9_]+)\s*\(", text))
    for sym in ("pem_tiled_mxv_arg", "pem_tiled_mxv_arg_f32", "pem_tiled_reduce_arg", "pem_tiled_reduce_arg_f32", "pem_tiled_bfs_parents"):
        assert sym in declared and sym in pkg.ABI_SYMBOLS and hasattr(pkg.lib(), sym), sym
    assert tuple(pkg.ARG_KINDS) == ar.KINDS
    for k, name in enumerate(ar.KINDS):
        assert re.search(rf"\bPEM_ARG_{name.upper()}\s*=\s*{k}\b", text), name
    for m in ("mxv_arg", "reduce_arg", "bfs_parents"):
        assert callable(getattr(pkg.Tiled, m))


def test_cli_refuses_before_it_opens_a_device(pkg, tmp_path):
    """--argreduce / --bfs-parents: one line and exit code 1 for a bad spec and for what they do not combine with"""
    import importlib
    import subprocess
    hostio = importlib.import_module("pem_spgemm_amd.hostio")
    fa = tmp_path / "A.mtx"
    fa.write_text("%%MatrixMarket matrix coordinate real general\n2 2 2\n1 1 1.0\n2 2 2.0\n")
    for args, line in ((["--argreduce", "rows"], "--argreduce rows: want rows|cols:min|max; unknown op  (min, max). Exiting."),
                       (["--argreduce", "diag:min"], "--argreduce diag:min: unknown dimension diag (rows, cols). Exiting."),
                       (["--argreduce", "rows:lor"], "--argreduce rows:lor: want rows|cols:min|max; unknown op lor (min, max). Exiting."),
                       (["--argreduce", "rows:min", "--reduce", "rows"], "--argreduce does not combine with --reduce. Exiting."),
                       (["--argreduce", "rows:min", "--bfs", "1"], "--argreduce does not combine with --bfs. Exiting."),
                       (["--argreduce", "rows:min", "--gpus", "2"], "--argreduce does not combine with --gpus. Exiting."),
                       (["--argreduce", "rows:min", "--power", "2"], "--argreduce does not combine with --power. Exiting."),
                       (["--bfs-parents", "0"], "--bfs-parents 0: want a 1-based vertex number. Exiting."),
                       (["--bfs-parents", "1x"], "--bfs-parents 1x: want a 1-based vertex number. Exiting."),
                       (["--bfs-parents", "1", "--bfs", "1"], "--bfs-parents does not combine with --bfs. Exiting."),
                       (["--bfs-parents", "1", "--argreduce", "cols:max"], "--bfs-parents does not combine with --argreduce. Exiting."),
                       (["--bfs-parents", "1", "--reduce", "cols"], "--bfs-parents does not combine with --reduce. Exiting."),
                       (["--bfs-parents", "1", "--gpus", "2"], "--bfs-parents does not combine with --gpus. Exiting.")):
        out = subprocess.run([hostio.CLI_PATH, str(fa), "0", *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert out.returncode == 1 and out.stdout == line + "\n", (args, out.stdout, out.stderr)
