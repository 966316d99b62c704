"""Independent numpy statement of the semirings of step 3 (include/pem_spgemm.h pem_semiring).

C's structure is the symbolic product: entry (i, j) is stored when some k has A(i,k) and B(k,j) stored.  Its value reduces the
products over every such k:
  plus_times  sum of a * b (here a plain numpy sum: the device's fma chain is checked against the oracle elsewhere)
  min_plus    fmin over (a + b), starting from +inf
  max_plus    fmax over (a + b), starting from -inf
  max_times   fmax over (a * b), starting from -inf
  plus_pair   the number of products (values never read)
  lor_land    1 if some product has a != 0 and b != 0 (NaN != 0), else 0
Each a + b / a * b is rounded once in the value type (numpy arithmetic on arrays of that dtype); fmin / fmax skip NaN, so an entry
whose every product is NaN keeps the start value.  Min/max do not depend on the order of the products.

Inputs are CSR triples (rowptr, colidx, vals) with sorted columns; the product is formed in row blocks of at most `chunk`
scalar products, so the full-size stand-ins fit in memory.
"""
import numpy as np

SEMIRINGS = ("plus_times", "min_plus", "max_plus", "max_times", "plus_pair", "lor_land")
NEW = SEMIRINGS[1:]


def start(semiring, dtype):
    return {"min_plus": np.inf, "max_plus": -np.inf, "max_times": -np.inf}.get(semiring, 0.0)


def coo_to_csr(rows, cols, I, J, V):
    """sorted CSR of a COO matrix without duplicates"""
    I, J = np.asarray(I, np.int64), np.asarray(J, np.int64)
    order = np.lexsort((J, I))
    rp = np.zeros(rows + 1, np.int64)
    np.cumsum(np.bincount(I, minlength=rows), out=rp[1:])
    return rp, J[order], np.asarray(V)[order]


def transpose_csr(rows, cols, rp, ci, v):
    I = np.repeat(np.arange(rows, dtype=np.int64), np.diff(rp))
    return coo_to_csr(cols, rows, ci, I, v)


def _reduce(semiring, a, b, seg, dtype):
    """one value per segment (seg: start index of each run of equal keys)"""
    if semiring == "plus_pair":
        return np.diff(np.append(seg, len(a))).astype(dtype)
    if semiring == "lor_land":
        hit = ((a != 0) & (b != 0)).astype(np.int8)
        return np.maximum.reduceat(hit, seg).astype(dtype) if len(seg) else np.zeros(0, dtype)
    if semiring == "plus_times":
        return np.add.reduceat(a * b, seg).astype(dtype) if len(seg) else np.zeros(0, dtype)
    x = a + b if semiring in ("min_plus", "max_plus") else a * b
    if not len(seg):
        return np.zeros(0, dtype)
    if semiring == "min_plus":
        return np.fmin(np.fmin.reduceat(x, seg), dtype(np.inf))
    return np.fmax(np.fmax.reduceat(x, seg), dtype(-np.inf))


def spgemm(A, B, ncols, semiring, dtype=np.float64, chunk=1 << 22):
    """C = A (x) B under `semiring`; A, B: CSR triples; returns the CSR triple of C (values in dtype)"""
    dtype = np.dtype(dtype).type
    arp, aci, av = A
    brp, bci, bv = B
    av, bv = np.asarray(av).astype(dtype), np.asarray(bv).astype(dtype)
    nrows = len(arp) - 1
    blen = np.diff(brp)
    per_a = blen[aci]                                         # products of every A entry
    row_prod = np.concatenate([[0], np.cumsum(per_a)])[arp]   # products before each row
    rp_out = np.zeros(nrows + 1, np.int64)
    cols_out, vals_out = [], []
    r0 = 0
    while r0 < nrows:
        # rows [r0, r1): at most `chunk` products, at least one row
        r1 = int(np.searchsorted(row_prod, row_prod[r0] + chunk, side="right")) - 1
        r1 = min(max(r1, r0 + 1), nrows)
        e0, e1 = int(arp[r0]), int(arp[r1])
        cnt = per_a[e0:e1]
        tot = int(cnt.sum())
        if tot == 0:
            r0 = r1
            continue
        ae = np.repeat(np.arange(e0, e1, dtype=np.int64), cnt)
        first = np.repeat(np.cumsum(cnt) - cnt, cnt)
        be = np.repeat(brp[aci[e0:e1]], cnt) + (np.arange(tot, dtype=np.int64) - first)
        arow = np.repeat(np.arange(r0, r1, dtype=np.int64), np.diff(arp[r0:r1 + 1]))[ae - e0]
        key = arow * ncols + bci[be]
        order = np.argsort(key, kind="stable")                # (stable: ascending k inside an entry)
        key, ae, be = key[order], ae[order], be[order]
        seg = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
        ukey = key[seg]
        vals_out.append(_reduce(semiring, av[ae], bv[be], seg, dtype))
        cols_out.append(ukey % ncols)
        rp_out[r0 + 1:r1 + 1] += np.bincount(ukey // ncols - r0, minlength=r1 - r0)
        r0 = r1
    np.cumsum(rp_out, out=rp_out)
    ci = np.concatenate(cols_out) if cols_out else np.zeros(0, np.int64)
    v = np.concatenate(vals_out) if vals_out else np.zeros(0, dtype)
    return rp_out, ci, v


def filter_csr(rp, ci, v, ncols, MI, MJ, complement=False):
    """C restricted to M's stored positions (or to where M stores nothing)"""
    rows = np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))
    keys = rows * ncols + ci
    mk = np.unique(np.asarray(MI, np.int64) * ncols + np.asarray(MJ, np.int64))
    keep = np.isin(keys, mk) != complement
    out = np.zeros(len(rp), np.int64)
    np.cumsum(np.bincount(rows[keep], minlength=len(rp) - 1), out=out[1:])
    return out, ci[keep], v[keep]


def dense(rows, cols, I, J, V, semiring, dtype=np.float64, B=None):
    """brute force over dense arrays (tests only): (present, value) of every (i, j); B = (rows, cols, I, J, V) or A itself"""
    dtype = np.dtype(dtype).type
    Bs = B if B is not None else (rows, cols, I, J, V)
    pa = np.zeros((rows, cols), bool)
    va = np.zeros((rows, cols), dtype)
    pa[I, J] = True
    va[I, J] = np.asarray(V).astype(dtype)
    pb = np.zeros((Bs[0], Bs[1]), bool)
    vb = np.zeros((Bs[0], Bs[1]), dtype)
    pb[Bs[2], Bs[3]] = True
    vb[Bs[2], Bs[3]] = np.asarray(Bs[4]).astype(dtype)
    n = Bs[1]
    present = np.zeros((rows, n), bool)
    val = np.zeros((rows, n), dtype)
    for i in range(rows):
        for j in range(n):
            acc = dtype(start(semiring, dtype))
            for k in range(cols):
                if not (pa[i, k] and pb[k, j]):
                    continue
                present[i, j] = True
                a, b = va[i, k], vb[k, j]
                if semiring == "plus_times":
                    acc = dtype(acc + a * b)
                elif semiring == "min_plus":
                    acc = np.fmin(acc, dtype(a + b))
                elif semiring == "max_plus":
                    acc = np.fmax(acc, dtype(a + b))
                elif semiring == "max_times":
                    acc = np.fmax(acc, dtype(a * b))
                elif semiring == "plus_pair":
                    acc = dtype(acc + 1)
                elif semiring == "lor_land":
                    acc = dtype(1) if (a != 0 and b != 0) else acc
            val[i, j] = acc
    return present, val


def same_values(got, want):
    """exact equality with -0 == +0 (and NaN == NaN, which the min/max semirings never produce)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return False
    both_nan = np.isnan(got) & np.isnan(want)
    return bool(np.all((got == want) | both_nan))
