"""CPU: tests/concatref.py against np.block of the dense forms (values by bits, null cells, zero-size strips, 1 x 1 blocks, one
operand in several cells), the split(concat) identity and the refresh's gather stated on the reference; the header's declarations
and the library's exports; the binding's argument errors, which come before any device call; the CLI's refusals of --hstack /
--vstack that need no device (the wrong-shape refusal needs the result and is in tests/test_gpu_concat.py)."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import concatref

DTYPES = (np.float64, np.float32)
IDS = ("f64", "f32")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pem_spgemm.h")
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3.0e-310, 1.0e-40, 0.5, -0.5])


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _sparse(rng, rows, cols, n, dt):
    """canonical (I, J, V), about a third of the values special (zeros are entries like any other)"""
    keys = np.sort(rng.choice(rows * cols, size=min(n, rows * cols), replace=False))
    V = rng.normal(size=len(keys))
    sp = rng.random(len(keys)) < 0.35
    V[sp] = rng.choice(SPECIAL, int(sp.sum()))
    return (keys // cols).astype(np.int32), (keys % cols).astype(np.int32), np.asarray(V, dt)


def _dense_pair(rows, cols, blk, dt):
    """(the stored flags, the values' bits) of a block's dense form; a null block stores nothing"""
    stored, bits = np.zeros((rows, cols), bool), np.zeros((rows, cols), np.uint64)
    if blk is not None:
        stored[blk[0], blk[1]] = True
        bits[blk[0], blk[1]] = _bits(np.asarray(blk[2], dt))
    return stored, bits


def _grids(rng, dt):
    """name -> (blocks, row_sizes, col_sizes)"""
    out = {}
    A, B, Cm, D = _sparse(rng, 5, 7, 12, dt), _sparse(rng, 5, 3, 9, dt), _sparse(rng, 4, 7, 10, dt), _sparse(rng, 4, 3, 12, dt)
    out["2x2"] = ([[A, B], [Cm, D]], (5, 4), (7, 3))
    out["nulls"] = ([[A, None], [None, D]], (5, 4), (7, 3))
    out["null_strips"] = ([[None, None, None], [None, A, None], [None, None, None]], (17, 5, 3), (16, 7, 2))
    out["zero_strips"] = ([[None, None, None], [A, None, B], [None, None, None]], (0, 5, 0), (7, 0, 3))
    S = _sparse(rng, 6, 6, 14, dt)
    out["aliased"] = ([[S, S], [S, S]], (6, 6), (6, 6))
    out["diag_aliased"] = ([[S, None], [None, S]], (6, 6), (6, 6))
    one = lambda: (np.zeros(1, np.int32), np.zeros(1, np.int32), np.asarray(rng.choice(SPECIAL, 1), dt))
    empty = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, dt))
    cells = [[(None, empty, one(), one())[int(rng.integers(0, 4))] for _ in range(20)] for _ in range(20)]
    cells[0][0] = one()
    out["ones_20x20"] = (cells, (1,) * 20, (1,) * 20)
    out["copy"] = ([[A]], (5,), (7,))
    out["hstack"] = ([[A, B, _sparse(rng, 5, 1, 3, dt)]], (5,), (7, 3, 1))
    out["vstack"] = ([[B], [D], [_sparse(rng, 1, 3, 2, dt)]], (5, 4, 1), (3,))
    out["all_empty"] = ([[empty, None], [empty, empty]], (3, 2), (4, 1))
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_concat_equals_numpys_block_of_the_dense_forms(dtype):
    rng = np.random.default_rng(11)
    for name, (blocks, rs, cs) in _grids(rng, dtype).items():
        rows, cols, I, J, V = concatref.concat(blocks, rs, cs, dtype)
        assert (rows, cols) == (sum(rs), sum(cs)) and V.dtype == np.dtype(dtype) and I.dtype == J.dtype == np.int32, name
        key = I.astype(np.int64) * max(cols, 1) + J
        assert np.all(np.diff(key) > 0), f"{name}: canonical: sorted, no duplicates"
        assert len(I) == sum(len(b[0]) for row in blocks for b in row if b is not None), name
        pairs = [[_dense_pair(rs[a], cs[b], blk, dtype) for b, blk in enumerate(row)] for a, row in enumerate(blocks)]
        want_stored = np.block([[p[0] for p in row] for row in pairs])
        want_bits = np.block([[p[1] for p in row] for row in pairs])
        assert want_stored.shape == (rows, cols), name
        got = np.zeros((rows, cols), bool)
        got[I, J] = True
        assert np.array_equal(got, want_stored), name
        assert np.array_equal(_bits(V).astype(np.uint64), want_bits[I, J]), f"{name}: values by bits"
        if name == "copy":
            assert all(np.array_equal(x, y) for x, y in zip((I, J, _bits(V)), (blocks[0][0][0], blocks[0][0][1], _bits(blocks[0][0][2]))))
        if name == "all_empty":
            assert len(I) == 0 and (rows, cols) == (5, 5)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_split_of_concat_is_the_grid(dtype):
    rng = np.random.default_rng(12)
    for name, (blocks, rs, cs) in _grids(rng, dtype).items():
        rows, cols, I, J, V = concatref.concat(blocks, rs, cs, dtype)
        pieces = concatref.split(I, J, V, rs, cs)
        for a, row in enumerate(blocks):
            for b, blk in enumerate(row):
                pI, pJ, pV = pieces[a][b]
                if blk is None:
                    assert len(pI) == 0, (name, a, b)
                else:
                    assert np.array_equal(pI, blk[0]) and np.array_equal(pJ, blk[1]) and np.array_equal(_bits(pV), _bits(np.asarray(blk[2], dtype))), \
                        (name, a, b)
        # ... and concat of the split of any matrix, cut anywhere, is the matrix
    I, J, V = _sparse(rng, 23, 31, 200, dtype)
    for rs, cs in (((23,), (31,)), ((1, 15, 7), (16, 15)), ((10, 0, 13), (0, 30, 1, 0))):
        pieces = concatref.split(I, J, V, rs, cs)
        rows, cols, bI, bJ, bV = concatref.concat(pieces, rs, cs, dtype)
        assert (rows, cols) == (23, 31) and np.array_equal(bI, I) and np.array_equal(bJ, J) and np.array_equal(_bits(bV), _bits(V))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_gather_is_the_refresh(dtype):
    rng = np.random.default_rng(13)
    for name, (blocks, rs, cs) in _grids(rng, dtype).items():
        flat = [blk for row in blocks for blk in row]
        cell, slot = concatref.gather(blocks, rs, cs)
        _, _, I, J, V = concatref.concat(blocks, rs, cs, dtype)
        assert len(cell) == len(V)
        assert all(flat[c] is not None for c in cell), name
        assert np.array_equal(_bits(V), _bits(np.array([np.asarray(flat[c][2], dtype)[s] for c, s in zip(cell, slot)], dtype))), name
        # new values on every block (one object in several cells gets one set): a refresh equals a fresh concat
        fresh = {}
        new_blocks = [[None if blk is None else (blk[0], blk[1], fresh.setdefault(id(blk), np.asarray(rng.choice(SPECIAL, len(blk[0])), dtype)))
                       for blk in row] for row in blocks]
        values = [None if blk is None else blk[2] for row in new_blocks for blk in row]
        want = concatref.concat(new_blocks, rs, cs, dtype)[4]
        assert np.array_equal(_bits(concatref.refreshed(blocks, rs, cs, values, dtype)), _bits(want)), name


def test_the_reference_refuses_what_it_cannot_state():
    A = (np.array([0, 4], np.int32), np.array([1, 6], np.int32), np.ones(2))
    with pytest.raises(ValueError):
        concatref.concat([[A]], (4,), (7,))                      # the block does not fit
    with pytest.raises(ValueError):
        concatref.concat([[A]], (5, 1), (7,))                    # the grid does not match the sizes
    with pytest.raises(ValueError):
        concatref.concat([[None]], (5,), (7,))
    with pytest.raises(ValueError):
        concatref.concat([[A]], (-5,), (7,))
    with pytest.raises(OverflowError):
        concatref.concat([[A, None]], (5,), (7, 2 ** 31 - 7))


def test_library_exports_and_header_declares(pkg):
    for sym in ("pem_tiled_concat", "pem_tiled_set_values_from_concat"):
        assert sym in pkg.ABI_SYMBOLS
        assert hasattr(pkg.lib(), sym), f"the library does not export {sym}"
    text = open(HEADER).read()
    assert re.search(r"pem_status\s+pem_tiled_concat\(pem_ctx \*ctx, int grid_rows, int grid_cols, const pem_tiled \*const \*blocks, "
                     r"const int64_t \*row_sizes,\s+const int64_t \*col_sizes, pem_tiled \*\*out\);", text)
    assert re.search(r"pem_status\s+pem_tiled_set_values_from_concat\(pem_ctx \*ctx, pem_tiled \*t, int nblocks, const pem_tiled \*const \*blocks\);", text)
    for name in ("concat", "hstack", "vstack", "set_values_from_concat", "split"):
        assert callable(getattr(pkg.Tiled, name)), name
    assert "extract" in pkg.Tiled.split.__doc__ and "no kernel of its own" in pkg.Tiled.split.__doc__


# ---- the binding's refusals that need no device ------------------------------------------------------------------------------
def _fake(pkg, rows, cols, value_bytes=8, ctx="ctx"):
    """a Tiled without a handle: every refusal below comes before the library is touched"""
    t = object.__new__(pkg.Tiled)
    t.rows, t.cols, t.value_bytes, t.ctx, t._h = rows, cols, value_bytes, ctx, None
    return t


def test_binding_value_errors(pkg, monkeypatch):
    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(pkg, "lib", no_library)
    T = pkg.Tiled
    A, B, D = _fake(pkg, 5, 7), _fake(pkg, 5, 3), _fake(pkg, 4, 3)
    bad = (
        (dict(blocks=[[A, B], [D]]), "rectangular"),                                    # ragged
        (dict(blocks=[]), "non-empty"),
        (dict(blocks=[[]]), "rectangular"),
        (dict(blocks=[A, B]), "list of lists"),
        (dict(blocks=[[A, 3]]), "Tiled or None"),
        (dict(blocks=[[None, None]]), "every block is None"),
        (dict(blocks=[[None, None]], row_sizes=[5], col_sizes=[3, 4]), "every block is None"),
        (dict(blocks=[[A, None], [None, None]]), "grid row 1 holds only None"),       # undeterminable sizes
        (dict(blocks=[[A, None], [None, None]], row_sizes=[5, 4]), "grid col 1 holds only None"),
        (dict(blocks=[[A, B], [None, D]], row_sizes=[5, 5]), "row_sizes[1] = 5"),      # contradicting sizes
        (dict(blocks=[[A, B], [None, D]], col_sizes=[8, 3]), "col_sizes[0] = 8"),
        (dict(blocks=[[A, B]], row_sizes=[5, 4]), "row_sizes must hold 1 sizes"),
        (dict(blocks=[[A, B]], col_sizes=[7, -3]), "col_sizes must hold 2 sizes"),
        (dict(blocks=[[A, D]]), "grid row 0 have [4, 5] rows"),                         # blocks that disagree
        (dict(blocks=[[B], [A]]), "grid col 0 have [3, 7] cols"),
        (dict(blocks=[[A, _fake(pkg, 5, 3, 4)]]), "different dtypes"),                  # mixed dtypes
        (dict(blocks=[[A, _fake(pkg, 5, 3, 8, "other")]]), "different contexts"),
    )
    for kwargs, word in bad:
        with pytest.raises(ValueError) as e:
            T.concat(**kwargs)
        assert word in str(e.value), (kwargs, str(e.value))
    with pytest.raises(ValueError):
        T.hstack([A, D])
    with pytest.raises(ValueError):
        T.vstack([A, B])
    # what passes the checks: the sizes come from the blocks, or are given for the strips of None
    assert T._concat_grid([[A, B], [None, D]])[3:] == ([5, 4], [7, 3])
    assert T._concat_grid([[None, None], [A, None]], row_sizes=[0, 5], col_sizes=[7, 16])[:2] == (2, 2)
    # split: the sizes sum to the shape and are at least 1
    for rs, cs in (((2, 2), (7,)), ((5,), (3, 3)), ((5, 0), (7,)), ((), (7,)), ((6, -1), (7,))):
        with pytest.raises(ValueError):
            T.split(A, rs, cs)


# ---- the CLI's refusals, before a device is opened ---------------------------------------------------------------------------
REFUSALS = (
    (["--hstack", "F.mtx", "--gpus", "2"], "--hstack does not combine with --gpus. Exiting.\n"),
    (["--vstack", "F.mtx", "--gpus", "2"], "--vstack does not combine with --gpus. Exiting.\n"),
    (["--hstack", "F.mtx", "--vstack", "G.mtx"], "--hstack does not combine with --vstack. Exiting.\n"),
    (["--vstack", "G.mtx", "--hstack", "F.mtx"], "--hstack does not combine with --vstack. Exiting.\n"),
    # an earlier step of the validation chain speaks first
    (["--kron-op", "plus", "--hstack", "F.mtx", "--vstack", "G.mtx"], "--kron-op needs --kron <K.mtx>. Exiting.\n"),
)


@pytest.mark.parametrize("k", range(len(REFUSALS)), ids=["_".join(a[0]).replace("--", "") for a in REFUSALS])
def test_cli_refusal(k, pkg, tmp_path):
    args, message = REFUSALS[k]
    hostio = importlib.import_module("pem_spgemm_amd.hostio")
    out = subprocess.run([hostio.CLI_PATH, "A.mtx", "0", *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert out.stdout == message
    assert out.returncode == 1, out.stderr
