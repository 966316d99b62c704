"""CPU: the step-3 path cases of tests/s3cases.py reach what they claim, and the bit-exact check they feed has power.

Coverage: each case's plan arrays come from the oracle's plan (pruned as prune_ref restates it, masked as maskref does); the
model of s3cases.py walks step 3's waves, trips and band tiles over them and must report every path the case claims.  All
cases together reach every path.  test_gpu_s3_paths.py then runs the same cases on the device.

Power: the oracle's ascending-k chain is what the device is compared with, bit for bit.  The same product through a reordered
inner dimension, (A P)(P^T B), is a different chain: it must differ from the ascending one on a large share of the entries with
two or more products -- so a kernel that sums a tile's pairs or products out of order cannot pass.  And one A entry less must
change every entry it feeds and no other -- so a kernel that skips one product cannot pass.
"""
import numpy as np
import pytest

import s3cases
import semiringref as sr

CASES = s3cases.cases()


@pytest.fixture(scope="module")
def models(oracle):
    return {name: s3cases.model_of(oracle, c) for name, c in CASES.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_reaches_its_paths(models, name):
    m = models[name]
    case = CASES[name]
    assert case["reach"] <= set(s3cases.PATHS), sorted(case["reach"] - set(s3cases.PATHS))
    assert case["reach"] <= m["paths"], f"{name} misses {sorted(case['reach'] - m['paths'])}"
    assert m["natural_epw"] == s3cases.S3_CHUNK, "the 512-entry waves are not chosen at these sizes: forced by s3_epw only"
    if dict(case["opts"]).get("s3_epw", 0) == 0:
        assert m["epw"] == s3cases.S3_CHUNK


def test_every_path_is_reached(models):
    table = {p: sorted(n for n, m in models.items() if p in m["paths"]) for p in s3cases.PATHS}
    width = max(map(len, table))
    print("\nstep-3 path -> cases")
    for p, names in table.items():
        print(f"  {p:<{width}}  {', '.join(names)}")
    empty = [p for p, names in table.items() if not names]
    assert not empty, f"no case reaches {empty}"
    claimed = set().union(*(c["reach"] for c in CASES.values()))
    assert claimed == set(s3cases.PATHS), sorted(set(s3cases.PATHS) - claimed)


def test_case_list_holds_the_option_variants():
    opts = [dict(c["opts"]) for c in CASES.values()]
    for epw in (1, 2, 4):
        for xcd in (0, 1):
            assert any(o.get("s3_epw") == epw and o.get("s3_xcd", 1) == xcd for o in opts), (epw, xcd)
    for k, v in (("s3_mark", 0), ("s3_decode", 0), ("wide", 0), ("prune", 0), ("s3_band", 0), ("s3_idx64", 1)):
        assert any(o.get(k) == v for o in opts), k
    assert any(c["mask"] == "complement" for c in CASES.values())
    assert any(c["tile_rows"] and c["tile_rows"][0] > 0 for c in CASES.values())


def test_builder_gives_the_asked_layout(oracle):
    """tile t of C is (t, t); its pair count and entry count are the spec's (pruned: the dead pairs and empty tiles go)"""
    for name in ("shallow", "deep_band", "unpruned"):
        case = CASES[name]
        arr = s3cases.plan_arrays(oracle, case)
        spec = case["spec"]
        if dict(case["opts"]).get("prune", 1):
            spec = [s for s in spec if s[0] > 0]
            npairs = [s[1] for s in spec]
        else:
            npairs = [s[1] + (s[3] if len(s) > 3 else 0) + (s[0] == 0) for s in spec]
        assert np.array_equal(np.diff(arr["c_tile_nnz_ptr"]), [s[0] for s in spec]), name
        assert np.array_equal(np.diff(arr["pairs_offset"]), npairs), name
        assert np.array_equal(arr["c_tile_rowidx"], arr["c_tile_colidx"]), name


def _csr(oracle, ops, f32=False):
    a, b = ops["A"], ops["B"]
    if f32:
        a = a[:4] + (a[4].astype(np.float32).astype(np.float64),)
        b = b[:4] + (b[4].astype(np.float32).astype(np.float64),)
    return oracle.csr_spgemm(oracle.Csr(*a), oracle.Csr(*b), f32=f32).arrays()


def _products(ops):
    """products per C entry (plus_pair), in the order of the CSR"""
    A = sr.coo_to_csr(*ops["A"])
    B = sr.coo_to_csr(*ops["B"])
    return sr.spgemm(A, B, ops["B"][1], "plus_pair")[2]


@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("name", ["shallow", "deep_band"])
def test_reordered_inner_dimension_changes_the_chain(oracle, name, f32):
    ops, _ = s3cases.operands(CASES[name])
    rp, ci, v = _csr(oracle, ops, f32)
    # reverse the k tiles of every C tile: each tile's pairs are summed last to first
    npairs = ops["pairs"]
    perm = np.concatenate([np.arange(k0 + n - 1, k0 - 1, -1) for k0, n in zip(np.cumsum([0] + npairs[:-1]), npairs)])
    assert len(perm) == ops["K"]
    rp2, ci2, v2 = _csr(oracle, s3cases.permute_k(ops, perm), f32)
    assert np.array_equal(rp, rp2) and np.array_equal(ci, ci2)
    cnt = _products(ops)
    multi = cnt >= 2
    assert multi.sum() > 1000
    differ = v[multi] != v2[multi]
    assert np.allclose(v, v2, rtol=1e-4 if f32 else 1e-12, atol=1e-5 if f32 else 1e-13)   # the same product ...
    print(f"{name}: {differ.mean():.2f} of {multi.sum()} entries with 2+ products differ")
    assert differ.mean() > 0.25, f"{name}: only {differ.mean():.2f} of the multi-product entries differ"   # ... another chain
    assert np.array_equal(v[~multi], v2[~multi])                                    # (one product: one rounding)


@pytest.mark.parametrize("name", ["shallow", "deep_band"])
def test_one_product_less_changes_the_entries_it_feeds(oracle, name):
    ops, _ = s3cases.operands(CASES[name])
    rows, cols, I, J, V = ops["A"]
    brows, bcols, BI, BJ, BV = ops["B"]
    rp, ci, v = _csr(oracle, ops)
    rng = np.random.default_rng(5)
    B_by_row = np.argsort(BI, kind="stable")
    for x in rng.choice(len(I), 12, replace=False):
        keep = np.arange(len(I)) != x
        ops2 = dict(ops, A=(rows, cols, I[keep], J[keep], V[keep]))
        rp2, ci2, v2 = _csr(oracle, ops2)
        fed = set((int(I[x]) * bcols + BJ[B_by_row][BI[B_by_row] == J[x]].astype(np.int64)).tolist())
        k1 = np.repeat(np.arange(rows, dtype=np.int64), np.diff(rp)) * bcols + ci
        k2 = np.repeat(np.arange(rows, dtype=np.int64), np.diff(rp2)) * bcols + ci2
        d2 = dict(zip(k2.tolist(), v2.view(np.uint64).tolist()))
        for k, bits in zip(k1.tolist(), v.view(np.uint64).tolist()):
            if k in fed:
                assert d2.get(k) != bits, f"{name}: A entry {x} feeds C key {k}, which did not change"
            else:
                assert d2[k] == bits
