"""numpy restatement of the element-wise combination of two tilings (csrc/ewise.hip, pem_tiled_ewise).

Operands are canonical COO triples (rows sorted by (row, column), no duplicates) of one shape and dtype.  The result is the canonical
COO of op(alpha*a, beta*b) over the union or the intersection of the two patterns, computed in the operands' dtype with one rounding
per operation (fp32 stays np.float32 throughout)."""
import numpy as np

PATTERNS = ("union", "intersect")
OPS = ("plus", "times", "min", "max", "lor", "land")


def _scale(v, s, dt):
    v = np.asarray(v, dt)
    if s == 1.0:
        return v
    with np.errstate(all="ignore"):
        return (dt.type(s) * v).astype(dt)


def apply_op(op, a, b):
    """op on two arrays of one dtype, element by element"""
    dt = a.dtype
    with np.errstate(all="ignore"):
        if op == "plus":
            return (a + b).astype(dt)
        if op == "times":
            return (a * b).astype(dt)
        if op == "min":
            return np.fmin(a, b).astype(dt)
        if op == "max":
            return np.fmax(a, b).astype(dt)
        if op == "lor":
            return ((a != 0) | (b != 0)).astype(dt)
        if op == "land":
            return ((a != 0) & (b != 0)).astype(dt)
    raise ValueError(op)


def ewise(cols, a, b, op="plus", pattern="union", alpha=1.0, beta=1.0):
    """a, b: (I, J, V) canonical COO of a rows x cols matrix.  Returns the expected (I, J, V), canonical."""
    Ia, Ja, Va = (np.asarray(x) for x in a)
    Ib, Jb, Vb = (np.asarray(x) for x in b)
    dt = np.dtype(Va.dtype)
    assert Vb.dtype == dt, "A and B must share a value type"
    ka = Ia.astype(np.int64) * cols + Ja
    kb = Ib.astype(np.int64) * cols + Jb
    sa, sb = _scale(Va, alpha, dt), _scale(Vb, beta, dt)
    both, ia, ib = np.intersect1d(ka, kb, assume_unique=True, return_indices=True)
    vboth = apply_op(op, sa[ia], sb[ib])
    if pattern == "intersect":
        keys, vals = both, vboth
    else:
        only_a = np.setdiff1d(np.arange(len(ka)), ia)
        only_b = np.setdiff1d(np.arange(len(kb)), ib)
        keys = np.concatenate([both, ka[only_a], kb[only_b]])
        vals = np.concatenate([vboth, sa[only_a], sb[only_b]]).astype(dt)
        o = np.argsort(keys, kind="stable")
        keys, vals = keys[o], vals[o]
    return (keys // cols).astype(np.int32), (keys % cols).astype(np.int32), np.asarray(vals, dt)


def canonical(I, J, V, cols):
    """sort a COO triple by (row, column)"""
    o = np.argsort(np.asarray(I, np.int64) * cols + np.asarray(J), kind="stable")
    return np.asarray(I, np.int32)[o], np.asarray(J, np.int32)[o], np.asarray(V)[o]
