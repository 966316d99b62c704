"""CPU: tests/applyref.py against independent statements -- the oracle's serial CSR product diag(r) * A * diag(c) for TIMES, the
numpy min_plus product (semiringref) for PLUS, exact integer powers for powi, the IEEE results on the special values -- and the
package's list of ops and the library's exports."""
import numpy as np
import pytest

import applyref as ap
import semiringref

DTYPES = (np.float64, np.float32)
IDS = ("f64", "f32")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _matrix(rng, rows, cols, n, dt):
    keys = np.sort(rng.choice(rows * cols, size=min(n, rows * cols), replace=False))
    fin = np.array([0.0, -0.0, 3.0e-310, 1.0e-40, 0.5, -0.5, 2.0 ** 60])
    mix = lambda m: np.where(rng.random(m) < 0.3, rng.choice(fin, m), rng.normal(size=m)).astype(dt)
    return (keys // cols).astype(np.int32), (keys % cols).astype(np.int32), mix(len(keys)), mix(rows), mix(cols)


def _csr(rows, I, V):
    return np.concatenate([[0], np.cumsum(np.bincount(I, minlength=rows))]).astype(np.int32), V


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_times_scale_is_the_oracles_diagonal_product(oracle, dtype):
    """diag(r) * A * diag(c) by two serial CSR products: a one-product fma from 0 is the product rounded once, so the values agree
    bit for bit wherever they are not zero (the fma's + 0 turns a -0 product into +0)"""
    f32 = dtype == np.float32
    rng = np.random.default_rng(5)
    for rows, cols, n in ((7, 9, 30), (40, 33, 500), (1, 50, 20), (50, 1, 20)):
        I, J, V, r, c = _matrix(rng, rows, cols, n, dtype)
        A = oracle.Csr(rows, cols, I, J, V.astype(np.float64))
        Dr = oracle.Csr(rows, rows, np.arange(rows), np.arange(rows), r.astype(np.float64))
        Dc = oracle.Csr(cols, cols, np.arange(cols), np.arange(cols), c.astype(np.float64))
        rp, ci, v = oracle.csr_spgemm(oracle.csr_spgemm(Dr, A, f32=f32), Dc, f32=f32).arrays()
        assert np.array_equal(ci, J) and np.array_equal(np.diff(rp), np.bincount(I, minlength=rows))
        got, want = ap.scale(I, J, V, r, c, "times", dtype), np.asarray(v).astype(dtype)
        assert got.dtype == np.dtype(dtype)
        assert np.all((_bits(got) == _bits(want)) | ((got == 0) & (want == 0)) | (np.isnan(got) & np.isnan(want)))
        # one side only
        rp, ci, v = oracle.csr_spgemm(Dr, A, f32=f32).arrays()
        got, want = ap.scale(I, J, V, r, None, "times", dtype), np.asarray(v).astype(dtype)
        assert np.all((_bits(got) == _bits(want)) | ((got == 0) & (want == 0)) | (np.isnan(got) & np.isnan(want)))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_plus_scale_is_the_min_plus_diagonal_product(dtype):
    """under min_plus diag(h) (x) A (x) diag(g) is fmin(inf, h_i + a_ij) and then + g_j: the reweighting, one rounding per sum"""
    rng = np.random.default_rng(6)
    for rows, cols, n in ((7, 9, 30), (40, 33, 500), (50, 1, 20)):
        I, J, V, r, c = _matrix(rng, rows, cols, n, dtype)
        rp = np.concatenate([[0], np.cumsum(np.bincount(I, minlength=rows))]).astype(np.int32)
        dr = (np.arange(rows + 1, dtype=np.int32), np.arange(rows, dtype=np.int32), r)
        dc = (np.arange(cols + 1, dtype=np.int32), np.arange(cols, dtype=np.int32), c)
        t = semiringref.spgemm(dr, (rp, J, V), cols, "min_plus", dtype)
        qp, qi, qv = semiringref.spgemm(t, dc, cols, "min_plus", dtype)
        assert np.array_equal(qp, rp) and np.array_equal(qi, J)
        got = ap.scale(I, J, V, r, c, "plus", dtype)
        assert np.all((_bits(got) == _bits(np.asarray(qv, dtype))) | ((got == 0) & (qv == 0)))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_powi_is_exact_on_small_integers_and_follows_the_chain(dtype):
    x = np.arange(-3, 4).astype(dtype)
    for k in range(1, 14):                       # |x|^k <= 3^13 < 2^24: exact in both types
        assert np.array_equal(ap.apply(x, "powi", k), np.array([int(v) ** k for v in range(-3, 4)], dtype)), k
    two = np.array([2.0, -2.0], dtype)
    assert np.array_equal(ap.apply(two, "powi", 64), np.array([2.0 ** 64, 2.0 ** 64], dtype))
    # the chain, spelled out for k = 5 = 0b101 and k = 6 = 0b110 on a value whose products round
    v = np.array([1.1, -0.7, 3.3e-5], dtype)
    sq = (v * v).astype(dtype)
    assert np.array_equal(_bits(ap.apply(v, "powi", 2)), _bits(sq))
    p4 = (sq * sq).astype(dtype)
    assert np.array_equal(_bits(ap.apply(v, "powi", 5)), _bits((p4 * v).astype(dtype)))
    p3 = (sq * v).astype(dtype)
    assert np.array_equal(_bits(ap.apply(v, "powi", 6)), _bits((p3 * p3).astype(dtype)))
    for k in (0, 65, 2.5, np.inf, -1, np.nan):
        assert not ap.powi_thunk_ok(k)
        with pytest.raises(ValueError):
            ap.apply(v, "powi", k)
    assert ap.powi_thunk_ok(1) and ap.powi_thunk_ok(64.0)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_identity_and_powi_one_copy_bit_for_bit(dtype):
    u = np.uint64 if dtype == np.float64 else np.uint32
    payload = np.array([0x7FF8000000000123, 0xFFF0000000000001, 0x7FF4000000000000] if dtype == np.float64 else
                       [0x7FC00123, 0xFF800001, 0x7FA00000], u).view(dtype)               # quiet and signalling NaNs with payloads
    v = np.concatenate([payload, np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, 1e-45, 1.5, -2.25]).astype(dtype)])
    for op, th in (("identity", 0), ("identity", 7.5), ("powi", 1)):
        assert np.array_equal(_bits(ap.apply(v, op, th)), _bits(v)), op
    # abs and ainv touch the sign bit only: payloads stay
    top = u(1) << u(8 * np.dtype(dtype).itemsize - 1)
    assert np.array_equal(_bits(ap.apply(v, "abs")), _bits(v) & ~top)
    assert np.array_equal(_bits(ap.apply(v, "ainv")), _bits(v) ^ top)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_unary_ops_on_the_specials(dtype):
    dt = np.dtype(dtype)
    tiny = dt.type(5e-324 if dtype == np.float64 else 1e-45)               # the smallest subnormal
    sub = dt.type(3.0e-310 if dtype == np.float64 else 1.0e-40)
    v = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, tiny, -tiny, sub, 4.0, -4.0], dt)
    inf = dt.type(np.inf)

    def same(got, want):
        want = np.array(want, dt)
        return got.dtype == dt and bool(np.all((_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))))

    assert same(ap.apply(v, "abs"), [0.0, 0.0, inf, inf, np.nan, tiny, tiny, sub, 4.0, 4.0])
    assert same(ap.apply(v, "ainv"), [-0.0, 0.0, -inf, inf, np.nan, -tiny, tiny, -sub, -4.0, 4.0])
    assert same(ap.apply(v, "minv"), [inf, -inf, 0.0, -0.0, np.nan, inf, -inf, inf, 0.25, -0.25])
    assert same(ap.apply(v, "sqrt"), [0.0, -0.0, inf, np.nan, np.nan, np.sqrt(tiny), np.nan, np.sqrt(sub), 2.0, np.nan])
    assert np.sqrt(tiny) > 0 and ap.apply(v, "div", 2.0)[7] == sub / dt.type(2) > 0   # subnormals are kept, not flushed
    assert same(ap.apply(v, "one"), [1.0] * len(v))
    assert same(ap.apply(v, "plus", np.nan), [np.nan] * len(v))           # a NaN thunk propagates ...
    assert same(ap.apply(v, "min", np.nan), v)                            # ... and min / max skip it
    assert same(ap.apply(v, "rdiv", 1.0), ap.apply(v, "minv"))
    assert same(ap.apply(v, "div", 0.0)[[8, 9, 0]], [inf, -inf, np.nan])
    assert same(ap.apply(v, "rminus", 1.0)[[8, 2]], [-3.0, -inf])
    # the thunk is rounded once to the value type
    x = np.array([1.0], dt)
    assert ap.apply(x, "times", 0.1)[0] == dt.type(0.1)
    # scale: a None vector's step is not performed; lor / land give 1.0 / 0.0 and NaN counts as != 0
    I, J = np.array([0, 0, 1], np.int32), np.array([0, 1, 1], np.int32)
    a = np.array([np.nan, 0.0, 2.0], dt)
    assert np.array_equal(_bits(ap.scale(I, J, a, None, None, "times")), _bits(a))
    assert same(ap.scale(I, J, a, np.array([0.0, 0.0], dt), None, "lor"), [1.0, 0.0, 1.0])
    assert same(ap.scale(I, J, a, np.array([1.0, 0.0], dt), np.array([1.0, 1.0], dt), "land"), [1.0, 0.0, 0.0])
    assert same(ap.scale(I, J, a, np.array([2.0, 3.0], dt), np.array([10.0, 100.0], dt), "plus"), [np.nan, 102.0, 105.0])


def test_package_lists_the_ops_and_library_exports_apply_and_scale(pkg):
    assert pkg.APPLY_OPS == ap.OPS
    assert len(pkg.APPLY_OPS) == 14
    assert tuple(sorted(pkg.BINOPS, key=pkg.BINOPS.get)) == ap.BINOPS
    for sym in ("pem_tiled_apply", "pem_tiled_set_values_from_apply", "pem_tiled_scale", "pem_tiled_scale_f32",
                "pem_tiled_set_values_from_scale", "pem_tiled_set_values_from_scale_f32"):
        assert sym in pkg.ABI_SYMBOLS
        assert hasattr(pkg.lib(), sym), f"the library does not export {sym}"


# ---- the CLI's refusals, all before a device is opened ----------------------------------------------------------------------------
ARRAY = "%%MatrixMarket matrix array real general\n"
CLI_REFUSALS = (
    (["--apply", "abs", "--gpus", "2"], ("--apply does not combine with --gpus",)),
    (["--apply", "abs", "--power", "3"], ("--apply does not combine with --power",)),
    (["--row-scale", "{v3}", "--gpus", "2"], ("--row-scale does not combine with --gpus",)),
    (["--col-scale", "{v3}", "--power", "3"], ("--col-scale does not combine with --power",)),
    (["--apply", "exp"], ("--apply exp", "unknown op exp", "identity, abs, ainv, minv, sqrt, one, plus, times, min, max, div, rdiv, rminus, powi")),
    (["--apply", "plus:1e-x"], ("--apply plus:1e-x", "does not parse as a number")),
    (["--apply", "times:"], ("does not parse as a number",)),
    (["--apply", "powi"], ("--apply powi", "needs an integral thunk k in 1 .. 64")),
    (["--apply", "powi:0"], ("needs an integral thunk k in 1 .. 64",)),
    (["--apply", "powi:65"], ("needs an integral thunk k in 1 .. 64",)),
    (["--apply", "powi:2.5"], ("needs an integral thunk k in 1 .. 64",)),
    (["--apply", "powi:nan"], ("needs an integral thunk k in 1 .. 64",)),
    (["--scale-op", "plus"], ("--scale-op needs --row-scale",)),
    (["--row-scale", "{v3}", "--scale-op", "minus"], ("--scale-op minus: unknown op (plus, times, min, max, lor, land)",)),
    (["--row-scale", "{v32}"], ("--row-scale", "an array of 2 columns, not of one")),
    (["--col-scale", "{v32}"], ("--col-scale", "an array of 2 columns, not of one")),
    (["--col-scale", "{none}"], ("--col-scale", "cannot open the file", "want a Matrix-Market array real general file")),
    (["--row-scale", "{short}"], ("--row-scale", "fewer values than rows x cols")),
    (["--row-scale", "{coord}"], ("--row-scale", "not an array (dense) file")),
)


@pytest.mark.parametrize("k", range(len(CLI_REFUSALS)), ids=["".join(a for a in r[0] if a.startswith("--")) + f"{k}" for k, r in enumerate(CLI_REFUSALS)])
def test_cli_refusal(k, pkg, tmp_path):
    import importlib
    import subprocess
    hostio = importlib.import_module("pem_spgemm_amd.hostio")
    files = dict(v3=ARRAY + "3 1\n1\n2\n3\n", v32=ARRAY + "3 2\n1\n2\n3\n1\n2\n3\n", short=ARRAY + "3 1\n1\n2\n",
                 coord="%%MatrixMarket matrix coordinate real general\n3 1 1\n1 1 2.0\n")
    for name, text in files.items():
        (tmp_path / f"{name}.mtx").write_text(text)
    args, words = CLI_REFUSALS[k]
    args = [a.format(none=tmp_path / "none.mtx", **{n: tmp_path / f"{n}.mtx" for n in files}) for a in args]
    out = subprocess.run([hostio.CLI_PATH, "A.mtx", "0", *args, "--out", str(tmp_path / "C.mtx")], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert out.returncode == 1, out.stdout + out.stderr
    for w in words:
        assert w in out.stdout, (w, out.stdout)
    assert out.stdout.rstrip().endswith("Exiting.") and not (tmp_path / "C.mtx").exists()
