"""CPU: the host reference of the sampled sparse product (tests/sampledref.py) against the oracle's A * B and the numpy semiring
product, its column-split identity, and the triangle-count formula.  Bit for bit over every entry (NaN == NaN; +0 == -0 under
min / max only).

S is A's pattern wherever A's shape is the product's (every square case); a non-square `_AAt` case has an m x m product, so its S
is a random m x m pattern with A's entry count.
"""
import importlib
import subprocess

import numpy as np
import pytest

import maskref
import sampledref as sr
import semiringref as sref

CASES, GENS, SMALL = sr.CASES, sr.GENS, sr.SMALL
DTYPES = (np.float64, np.float32)
MINMAX = ("min_plus", "max_plus", "max_times")


def _same(got, want, kind="plus_times"):
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    ok = (got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want))
    if kind in MINMAX:
        ok |= (got == 0) & (want == 0)
    return bool(np.all(ok))


problem = sr.problem


def _expect(S, C, p, semiring, dtype):
    """the product C (a CSR triple) at S's positions, the start value elsewhere"""
    SI, SJ = S
    crp, cci, cv = C
    keys = maskref.pattern_keys(sr.rows_of(crp), cci, p)
    o = np.argsort(keys)
    want = np.full(len(SI), sr.START[semiring], dtype)
    sk = maskref.pattern_keys(SI, SJ, p)
    pos = np.searchsorted(keys[o], sk)
    hit = pos < len(keys)
    hit[hit] = keys[o][pos[hit]] == sk[hit]
    want[hit] = np.asarray(cv).astype(dtype)[o][pos[hit]]
    # the same positions through maskref.filter_csr: the masked product's pattern is exactly the hits
    frp, fci, fv = maskref.filter_csr(crp, cci, cv, SI, SJ, p)
    assert int(frp[-1]) == int(hit.sum())
    return want, hit


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", SMALL + sorted(GENS))
def test_reference_equals_the_masked_product(oracle, name, dtype):
    m, n, p, S, A, B = problem(name)
    matched = sr.match(S[0], S[1], A, B, n, p)
    # plus_times: the oracle's A * B
    oa = oracle.Csr(m, n, sr.rows_of(A[0]), A[1], np.asarray(A[2], np.float64))
    ob = oracle.Csr(n, p, sr.rows_of(B[0]), B[1], np.asarray(B[2], np.float64))
    C = oracle.csr_spgemm(oa, ob, 1, f32=dtype == np.float32).arrays()
    want, hit = _expect(S, C, p, "plus_times", dtype)
    assert _same(sr.fold(matched, A, B, "plus_times", dtype, oracle=oracle), want), name
    assert np.array_equal(np.diff(matched[0]) > 0, hit), f"{name}: the entries some k reaches are the product's"
    # the five others: the numpy semiring product
    for s in sref.NEW:
        C = sref.spgemm(A, B, p, s, dtype)
        want, _ = _expect(S, C, p, s, dtype)
        assert _same(sr.fold(matched, A, B, s, dtype), want, s), f"{name} {s}"


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", ("rand_300", "rect_33x65_AAt", "band_1500", "long_lists", "ragged", "full_tile"))
def test_reference_column_split(oracle, name, dtype):
    """a call on (A1, B1) followed by an accumulate call on (A2, B2) is one call on (A, B)"""
    m, n, p, S, A, B = problem(name)
    for n1 in (0, 1, 16, n // 2, n - 1, n):
        (A1, B1), (A2, B2) = sr.split_columns(A, B, n1, p)
        for s in sr.SEMIRINGS:
            whole = sr.sampled(S[0], S[1], A, B, n, p, s, dtype, oracle=oracle)
            first = sr.sampled(S[0], S[1], A1, B1, n, p, s, dtype, oracle=oracle)
            both = sr.sampled(S[0], S[1], A2, B2, n, p, s, dtype, old=first, oracle=oracle)
            assert _same(both, whole, s), f"{name} {s} n1={n1}"


def test_long_list_positions():
    a, b = sr.long_list_keys()
    assert len(a) == 130 and len(b) == 70
    g = GENS["long_lists"]
    assert np.array_equal(np.unique(g["A"][1] // 16), a) and np.array_equal(np.unique(g["B"][0] // 16), b)


def test_triangle_formula():
    """sum(L o (L . L^T)) under plus_pair, L the strict lower triangle, is trace(A^3) / 6"""
    for n, I, J in (sr.triangle_graph(), (600,) + sr.symmetrised(600, CASES["powerlaw_600"][2], CASES["powerlaw_600"][3])):
        want = sr.triangles(n, I, J)
        low = I > J
        L = sr.csr(n, n, I[low], J[low], np.ones(int(low.sum())))
        LI = sr.rows_of(L[0])
        R = sr.sampled(LI, L[1], L, sr.transpose(n, n, L), n, n, "plus_pair", np.float64)
        assert int(R.sum()) == want and want > 0


def test_cli_refusals(pkg, tmp_path):
    """what the CLI refuses of the new flags before it opens a device: the message names the flag and what it met, exit code 1"""
    hostio = importlib.import_module("pem_spgemm_amd.hostio")
    a = tmp_path / "A.mtx"
    a.write_text("%%MatrixMarket matrix coordinate real general\n2 2 2\n1 1 1.0\n2 2 1.0\n")
    fa = str(a)
    takes = "(it takes the place of the plan product, and no stage runs after it)"
    cases = [([fa, "0", "--sampled-bt"], "--sampled-bt needs --sampled <S.mtx>. Exiting.\n"),
             ([fa, "0", "--sampled", fa, "--triangles"], "--triangles does not combine with --sampled"),
             ([fa, "0", "1", "--sampled", fa, "--sampled-bt"], "--sampled-bt does not combine with the A*A^T argument"),
             ([fa, "1", "--sampled", fa], f"--sampled does not combine with the 2nd argument 1 (the sorted COO files; use --out) {takes}"),
             ([fa, "0", "--triangles", "--B", fa], "--triangles does not combine with --B"),
             ([fa, "0", "1", "--triangles"], "--triangles does not combine with the A*A^T argument"),
             ([fa, "0", "--triangles", "--semiring", "plus_pair"], "--triangles does not combine with --semiring"),
             ([fa, "0", "--triangles", "--out", str(tmp_path / "o.mtx")], "--triangles does not combine with --out"),
             ([fa, "0", "--sampled", fa, "--semiring", "plus_min"], "--semiring plus_min: unknown semiring")]
    for flag, value in (("--gpus", "2"), ("--mask", fa), ("--power", "2"), ("--add", fa), ("--apply", "abs"), ("--select", "tril:0"),
                        ("--topk", "rows:largest:1"), ("--assign-into", fa), ("--kron", fa), ("--hstack", fa), ("--vstack", fa),
                        ("--reduce", "rows"), ("--bfs", "1"), ("--argreduce", "rows:max"), ("--bfs-parents", "1"), ("--cache", str(tmp_path))):
        for new in (["--sampled", fa], ["--triangles"]):
            cases.append(([fa, "0", *new, flag, value], f"{new[0]} does not combine with {flag} {takes}. Exiting.\n"))
    for args, want in cases:
        out = subprocess.run([hostio.CLI_PATH, *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert out.returncode == 1 and want in out.stdout, (args, out.stdout, out.stderr)
        assert out.stdout.count("\n") == 1, (args, out.stdout)
