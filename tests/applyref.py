"""numpy restatement of apply and scale (csrc/apply.hip, pem_tiled_apply / pem_tiled_scale).

Both keep the pattern and change only the values, so they work on the value array of a COO triple (and, for scale, its coordinates):
everything is computed in the operand's dtype with one rounding per operation (fp32 stays np.float32 throughout; numpy's divide and
sqrt are IEEE correctly rounded and keep subnormals)."""
import numpy as np

from ewiseref import apply_op

OPS = ("identity", "abs", "ainv", "minv", "sqrt", "one", "plus", "times", "min", "max", "div", "rdiv", "rminus", "powi")
UNARY = OPS[:6]
BINOPS = ("plus", "times", "min", "max", "lor", "land")


def powi_thunk_ok(thunk):
    """the rule of PEM_APPLY_POWI: an integer k in 1..64"""
    t = float(thunk)
    return np.isfinite(t) and t == np.floor(t) and 1.0 <= t <= 64.0


def powi(x, k):
    """x^k by the stated chain: the bits of k below its leading one, from the top: p = p*p, then p = p*x if the bit is set"""
    x = np.asarray(x)
    dt = x.dtype
    p = x.copy()
    with np.errstate(all="ignore"):
        for b in bin(int(k))[3:]:
            p = (p * p).astype(dt)
            if b == "1":
                p = (p * x).astype(dt)
    return p


def _flip_sign(v, clear):
    u = v.view(np.uint64 if v.dtype == np.float64 else np.uint32).copy()
    top = u.dtype.type(1) << u.dtype.type(8 * u.dtype.itemsize - 1)
    return (u & ~top if clear else u ^ top).view(v.dtype)


def apply(V, op, thunk=0.0, dtype=None):
    """the values op gives for the values V; y = the thunk rounded once to the dtype"""
    dt = np.dtype(dtype if dtype is not None else np.asarray(V).dtype)
    v = np.ascontiguousarray(V, dt)
    if op not in OPS:
        raise ValueError(f"unknown apply op {op!r}")
    if op == "powi":
        if not powi_thunk_ok(thunk):
            raise ValueError(f"the thunk of powi must be an integer in 1..64, not {thunk!r}")
        return powi(v, int(thunk))
    with np.errstate(all="ignore"):
        y = dt.type(thunk)
        one = dt.type(1)
        if op == "identity":
            return v.copy()
        if op == "abs":
            return _flip_sign(v, True)
        if op == "ainv":
            return _flip_sign(v, False)
        if op == "minv":
            return (one / v).astype(dt)
        if op == "sqrt":
            return np.sqrt(v).astype(dt)
        if op == "one":
            return np.ones(len(v), dt)
        if op == "plus":
            return (v + y).astype(dt)
        if op == "times":
            return (v * y).astype(dt)
        if op == "min":
            return np.fmin(v, y).astype(dt)
        if op == "max":
            return np.fmax(v, y).astype(dt)
        if op == "div":
            return (v / y).astype(dt)
        if op == "rdiv":
            return (y / v).astype(dt)
        return (y - v).astype(dt)   # rminus


def scale(I, J, V, r=None, c=None, op="times", dtype=None):
    """z = op(op(r[i], a), c[j]) left to right; a None vector's step is not performed"""
    dt = np.dtype(dtype if dtype is not None else np.asarray(V).dtype)
    z = np.ascontiguousarray(V, dt).copy()
    if op not in BINOPS:
        raise ValueError(f"unknown scale op {op!r}")
    if r is not None:
        z = apply_op(op, np.asarray(r, dt)[np.asarray(I, np.int64)], z)
    if c is not None:
        z = apply_op(op, z, np.asarray(c, dt)[np.asarray(J, np.int64)])
    return np.asarray(z, dt)
