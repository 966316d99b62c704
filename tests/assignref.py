"""numpy restatement of assign (csrc/assign.hip, pem_tiled_assign).

C and A are COO triples (I, J, V) of the rows x cols matrix C and of the ni x nj matrix A (no duplicate positions, one dtype) plus the
index lists RI and CJ (None = all, in order; no index repeated).  The result is the canonical COO -- sorted by (row, column) -- of Z:
outside RI x CJ what C stores; inside, without an accum, (RI[p], CJ[q]) exactly where A stores (p, q), with A's value; with an accum
the union of C's and A's entries there, accum(c, a) where both store one (ewiseref.apply_op: one rounding in the dtype) and the one
stored value unchanged elsewhere.  Values are moved by index or go through apply_op, so every bit pattern a copy carries survives."""
import numpy as np

import ewiseref as ew


def check_list(L, dim, name="list"):
    """the rule of pem_tiled_assign for a non-null list: 1 .. INT32_MAX integer indices, each in 0 .. dim - 1, none repeated"""
    L = np.asarray(L)
    if L.ndim != 1 or L.size < 1 or L.size > 2 ** 31 - 1:
        raise ValueError(f"{name}: want 1 .. INT32_MAX indices, got shape {L.shape}")
    if L.dtype.kind not in "iu":
        raise ValueError(f"{name}: indices must be integers, not {L.dtype}")
    if int(L.min()) < 0 or int(L.max()) >= dim:
        raise ValueError(f"{name}: an index is outside 0 .. {dim - 1}")
    if len(np.unique(L)) != len(L):
        raise ValueError(f"{name}: an index is repeated")
    return L.astype(np.int64)


def assign(rows, cols, C, A, RI=None, CJ=None, accum=None):
    """(I', J', V'): the canonical COO of Z; I', J' int32, V' in the operands' dtype"""
    Ic, Jc, Vc = np.asarray(C[0], np.int64), np.asarray(C[1], np.int64), np.asarray(C[2])
    Ia, Ja, Va = np.asarray(A[0], np.int64), np.asarray(A[1], np.int64), np.asarray(A[2])
    dt = np.dtype(Vc.dtype)
    if np.dtype(Va.dtype) != dt:
        raise ValueError("C and A must share a value type")
    if accum is not None and accum not in ew.OPS:
        raise ValueError(f"unknown accum {accum!r}")
    RI = np.arange(rows, dtype=np.int64) if RI is None else check_list(RI, rows, "rows")
    CJ = np.arange(cols, dtype=np.int64) if CJ is None else check_list(CJ, cols, "cols")
    if len(Ia) and (int(Ia.max()) >= len(RI) or int(Ja.max()) >= len(CJ)):
        raise ValueError("A does not fit the region")
    oc = np.argsort(Ic * cols + Jc, kind="stable")
    Ic, Jc, Vc = Ic[oc], Jc[oc], Vc[oc]
    # A's entries at their destinations, canonical
    Is, Js = RI[Ia], CJ[Ja]
    o = np.argsort(Is * cols + Js, kind="stable")
    S = (Is[o].astype(np.int32), Js[o].astype(np.int32), Va[o])
    if accum is not None:
        return ew.ewise(cols, (Ic.astype(np.int32), Jc.astype(np.int32), Vc), S, op=accum, pattern="union")
    in_r, in_c = np.zeros(rows, bool), np.zeros(cols, bool)
    in_r[RI] = True
    in_c[CJ] = True
    keep = ~(in_r[Ic] & in_c[Jc])                        # C's entries outside the region
    keys = np.concatenate([Ic[keep] * cols + Jc[keep], S[0].astype(np.int64) * cols + S[1]])
    vals = np.concatenate([Vc[keep], S[2]]).astype(dt)
    o = np.argsort(keys, kind="stable")
    return (keys[o] // cols).astype(np.int32), (keys[o] % cols).astype(np.int32), vals[o]
