"""CPU: the numpy restatement of the masked product (tests/maskref.py) against a dense brute force.

The restatement is what the GPU tests hold the masked plans to, so it is checked here on its own: applied to the tiled oracle's
unmasked lists (the reference's, no pruning) it must give exactly pattern(A*B) intersected with pattern(M) -- or with its
complement -- and keep every kept tile's pairs as they were.
"""
import zlib

import numpy as np
import pytest

import maskref


def _rand(rng, r, c, nz):
    key = rng.choice(r * c, min(nz, r * c), replace=False)
    return (key // c).astype(np.int32), (key % c).astype(np.int32), rng.uniform(-1, 1, len(key))


def _dense_pattern(r, c, I, J):
    d = np.zeros((r, c), bool)
    d[I, J] = True
    return d


def _masks(rng, r, c, A_pat):
    """name -> (I, J) of M: empty, sparse random, dense tiles, partial tiles, A's own pattern (square only)"""
    out = {"empty": (np.zeros(0, np.int32), np.zeros(0, np.int32))}
    I, J, _ = _rand(rng, r, c, max(1, r * c // 20))
    out["sparse"] = (I, J)
    d = np.zeros((r, c), bool)
    for ti in range(0, r, 16):
        for tj in range(0, c, 16):
            u = rng.random()
            if u < 0.3:
                d[ti:ti + 16, tj:tj + 16] = True                 # a full tile (clipped at the edges)
            elif u < 0.6:
                d[ti:ti + 16, tj:tj + 16] = rng.random(d[ti:ti + 16, tj:tj + 16].shape) < 0.5
    out["tiles"] = tuple(a.astype(np.int32) for a in np.nonzero(d))
    if A_pat is not None:
        out["A"] = tuple(a.astype(np.int32) for a in np.nonzero(A_pat))
    return out


def _decode(res, ncols_c):
    """(row, col) keys of every entry of the restated masked plan"""
    m = res["c_mask"].reshape(-1, 8)
    keys = []
    for k in range(res["ntiles_c"]):
        ti, tj = int(res["c_tile_rowidx"][k]), int(res["c_tile_colidx"][k])
        for q in range(8):
            for rr, row in ((2 * q, m[k, q] >> 16), (2 * q + 1, m[k, q] & 0xFFFF)):
                for cc in range(16):
                    if (int(row) >> cc) & 1:
                        keys.append((16 * ti + rr) * ncols_c + 16 * tj + cc)
    return np.sort(np.array(keys, np.int64))


SHAPES = [("square_60", 60, 60, 60, 500, False), ("square_100_dense", 100, 100, 100, 3000, False),
          ("rect_AAt_50x37", 50, 37, 50, 400, True), ("ragged_33", 33, 33, 33, 200, False)]


@pytest.mark.parametrize("name,m,k,n,nz,aat", SHAPES, ids=[s[0] for s in SHAPES])
@pytest.mark.parametrize("complement", [False, True])
def test_restatement_matches_dense_brute_force(oracle, name, m, k, n, nz, aat, complement):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    AI, AJ, AV = _rand(rng, m, k, nz)
    AV[::7] = 0.0                                                 # explicit zeros are entries
    A = oracle.Tiled(m, k, AI, AJ, AV)
    if aat:
        B = oracle.Tiled(m, k, AI, AJ, AV, True)
        B_pat = _dense_pattern(m, k, AI, AJ).T
    else:
        BI, BJ, BV = _rand(rng, k, n, nz)
        B = oracle.Tiled(k, n, BI, BJ, BV)
        B_pat = _dense_pattern(k, n, BI, BJ)
    A_pat = _dense_pattern(m, k, AI, AJ)
    P = (A_pat.astype(np.int64) @ B_pat.astype(np.int64)) > 0     # symbolic pattern of A*B
    nc = P.shape[1]
    plan = oracle.Plan(A, B)
    for mname, (MI, MJ) in _masks(rng, m, nc, A_pat if m == k == nc else None).items():
        M = oracle.Tiled(m, nc, MI, MJ, np.zeros(len(MI)))        # values never matter (explicit zeros included)
        res = maskref.restate(plan, M, complement)
        M_pat = _dense_pattern(m, nc, MI, MJ)
        want = P & (~M_pat if complement else M_pat)
        wr, wc = np.nonzero(want)
        assert np.array_equal(_decode(res, nc), wr.astype(np.int64) * nc + wc), f"{name} {mname} complement={complement}"
        assert res["nnz_c"] == want.sum() and res["c_tile_nnz_ptr"][-1] == res["nnz_c"]
        # kept tiles: M holds them (normal) / M does not hold them full (complement); every kept tile keeps its pairs
        mt = res["c_mtile"]
        if complement:
            full = np.zeros(len(mt), bool)
            full[mt >= 0] = np.all(maskref.m_packed(M.masks)[mt[mt >= 0]] == 0xFFFFFFFF, axis=1)
            assert not full.any()
        else:
            assert np.all(mt >= 0)
            m_row = np.repeat(np.arange(M.tile_rows), np.diff(M.tile_rowptr))     # (tile_rowidx is the column-major index)
            assert np.array_equal(m_row[mt], res["c_tile_rowidx"]) and np.array_equal(M.tile_colidx[mt], res["c_tile_colidx"])
        old = {(int(r), int(c)): t for t, (r, c) in enumerate(zip(plan.c_tile_rowidx, plan.c_tile_colidx))}
        for t in range(res["ntiles_c"]):
            o = old[(int(res["c_tile_rowidx"][t]), int(res["c_tile_colidx"][t]))]
            p0, p1 = res["pairs_offset"][t], res["pairs_offset"][t + 1]
            q0, q1 = plan.pairs_offset[o], plan.pairs_offset[o + 1]
            assert np.array_equal(res["pairs_a"][p0:p1], plan.pairs_a[q0:q1]) and np.array_equal(res["pairs_b"][p0:p1], plan.pairs_b[q0:q1])
        # the CSR filter agrees with the dense brute force on the oracle's C
        rp, ci, v = plan.export_csr()
        frp, fci, fv = maskref.filter_csr(rp, ci, v, MI, MJ, nc, complement)
        dense = np.zeros((m, nc), bool)
        dense[np.repeat(np.arange(m), np.diff(frp)), fci] = True
        assert np.array_equal(dense, want) and len(fci) == want.sum()


def test_row_range_restatement_concatenates(oracle):
    """Restating the slices of a row range (M's tile rows of the same global indices) gives the whole masked C's arrays."""
    rng = np.random.default_rng(5)
    I, J, V = _rand(rng, 90, 90, 900)
    A = oracle.Tiled(90, 90, I, J, V)
    MI, MJ, _ = _rand(rng, 90, 90, 2000)
    M = oracle.Tiled(90, 90, MI, MJ, np.ones(len(MI)))
    whole = maskref.restate(oracle.Plan(A, A), M)
    parts = [maskref.restate(oracle.Plan(A, A, lo, hi), M) for lo, hi in ((0, 2), (2, 5), (5, 6))]
    for key in ("c_tile_colidx", "c_mask", "c_mtile", "c_tile_rowidx"):
        assert np.array_equal(np.concatenate([p[key] for p in parts]), whole[key]), key
