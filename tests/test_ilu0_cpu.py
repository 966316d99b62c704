"""CPU: ilu0ref, the host statement of ILU(0), proved against what can be computed without it -- on the
pattern L U reproduces A within the standard backward-error bound -- and the binding's declarations."""
import os
import re

import numpy as np
import pytest

import ilu0cases as ic
import ilu0ref as ir
import trsvref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ic.cases()


def _residual(n, rp, ci, a, f, wide):
    """per stored (i, j): |(L U - A)_ij| and (|L| |U|)_ij, both accumulated in `wide`, which carries many more bits than the factor"""
    rp, ci = [int(p) for p in rp], [int(j) for j in ci]
    fw = [wide(x) for x in f]
    where = [dict((ci[e], e) for e in range(rp[i], rp[i + 1])) for i in range(n)]
    res, mag = np.zeros(len(ci)), np.zeros(len(ci))
    for i in range(n):
        for e in range(rp[i], rp[i + 1]):
            j = ci[e]
            m = min(i, j)
            last = fw[e] * fw[where[j][j]] if j < i else fw[e]   # l_ij u_jj, or 1 * u_ij
            s, t = last, abs(last)
            for ek in range(rp[i], rp[i + 1]):
                k = ci[ek]
                if k >= m:
                    break
                ekj = where[k].get(j)
                if ekj is not None:
                    p = fw[ek] * fw[ekj]
                    s, t = s + p, t + abs(p)
            res[e], mag[e] = float(abs(s - wide(a[e]))), float(t)
    return res, mag


@pytest.mark.parametrize("dtype", ic.DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_is_finite_and_backward_stable(name, dtype):
    """|(L U - A)_ij| <= gamma_(c+2) (|L| |U|)_ij on the pattern; gamma_m = m u / (1 - m u), u the unit roundoff, c the longest chain:
    c fmas, one division and the closing product, each one rounding (Higham, Accuracy and Stability, Theorem 9.3's argument)"""
    n, rp, ci, a = ic.csr(CASES[name], dtype)
    f, chain = ir.ilu0(n, rp, ci, a, dtype)
    assert f.dtype == np.dtype(dtype) and np.all(np.isfinite(f))
    u = float(np.finfo(dtype).eps) / 2
    m = chain + 2
    gamma = m * u / (1 - m * u)
    res, mag = _residual(n, rp, ci, a, f, np.float64 if dtype is np.float32 else np.longdouble)
    assert np.all(res <= gamma * mag), (name, chain, float(np.max(res / np.maximum(mag, 1e-300))) / gamma)


def test_chains_and_levels_are_the_ones_the_cases_are_for():
    chains = {name: ir.ilu0(*ic.csr(CASES[name]))[1] for name in ("dense_33", "tridiagonal_200", "double_arrow_400")}
    assert chains == {"dense_33": 32, "tridiagonal_200": 1, "double_arrow_400": 399}
    for name, ws in ic.WIDTHS.items():
        n, rp, ci, _ = ic.csr(CASES[name])
        assert tr.widths(tr.levels(n, rp, ci, "lower")) == ws, name
    n, I, J, V = CASES["double_arrow_400"]
    assert len(set((J[I // 16 == 24] // 16).tolist())) == 25   # the last tile row holds 25 tiles


def test_unstored_positions_are_not_zeros():
    """a_00 = 0 makes f_10 infinite; (0, 1) is not stored, so f_11 stays a_11 where a stored zero would have made it NaN"""
    rp, ci, v = [0, 1, 3, 4], [0, 0, 1, 2], [0.0, 1.0, 5.0, 2.0]
    f, _ = ir.ilu0(3, rp, ci, v)
    assert np.isinf(f[1]) and f[2] == 5.0
    f, _ = ir.ilu0(3, [0, 2, 4, 5], [0, 1, 0, 1, 2], [0.0, 0.0, 1.0, 5.0, 2.0])
    assert np.isnan(f[3])
    with pytest.raises(ValueError, match="row 2 "):
        ir.ilu0(3, [0, 1, 2, 3], [0, 0, 2], [1.0, 1.0, 1.0])


def test_header_and_binding_name_the_symbols(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pem_spgemm.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pem_[a-z0-9_]+)\s*\(", text))
    for sym in ("pem_tiled_ilu0", "pem_tiled_set_values_from_ilu0", "pem_tiled_ilu0_info"):
        assert sym in declared and sym in pkg.ABI_SYMBOLS and hasattr(pkg.lib(), sym), sym
    assert [f for f, _ in pkg.Ilu0Info._fields_] == ["levels", "launches", "max_width", "merge_width", "zero_pivots", "first_zero_pivot_row"]
    assert re.search(r"int64_t\s+levels,\s*launches,\s*max_width,\s*merge_width,\s*zero_pivots,\s*first_zero_pivot_row;\s*}\s*pem_ilu0_info", text)
    for m in ("ilu0", "set_values_from_ilu0", "ilu0_info", "lu_solve"):
        assert callable(getattr(pkg.Tiled, m))
