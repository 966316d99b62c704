"""Independent numpy statement of the Krylov solvers (include/pem_spgemm.h pem_krylov_solve): CG and
right-preconditioned BiCGStab, bit for bit.

Arithmetic.  VT = the value type.  Vector updates use no fma: every product and every sum is rounded once in VT (numpy arithmetic
on arrays of that dtype), in the order the header's parentheses give.  Scalars are fp64 (numpy float64 scalars, one IEEE operation
per operator); a scalar is rounded once to VT before it multiplies a vector.  A x is mxvref's fma chain, the LU preconditioner two
trsvref solves (lower with a unit diagonal, then upper).

dot(u, v): fp64 products (exact for fp32 inputs).  Chunks of 4096 elements; G = min(ceil(n / 4096), 1024) workgroups of 256
threads; workgroup g takes the chunks g, g + G, ...; thread t the elements chunk * 4096 + t + 256 j, j = 0 .. 15; one chain
acc = acc + u_i v_i from +0.0 in ascending i (an element past n adds +0.0, which changes no bit: a chain that starts at +0.0
never holds -0.0).  Lane l of a wave adds the acc of lane l xor m for m = 32 .. 1; the waves combine as (w0 + w1) + (w2 + w3).
The total chains partial[t], [t + 256], [t + 512], [t + 768] in thread t and runs the same tree.

The scalar logic below is the header's, line by line.
"""
import numpy as np

import mxvref
import trsvref

CHUNK, THREADS, PER, MAXG = 4096, 256, 16, 1024
CONVERGED, MAX_ITERS, BREAKDOWN, NONFINITE = 0, 1, 2, 3
STATUS = ("converged", "max_iters", "breakdown", "nonfinite")
_LANE = np.arange(64)


def grid(n):
    return max(1, min(-(-n // CHUNK), MAXG))


def _tree(acc):
    """acc: (..., 256) per-thread chains -> (...) the workgroup's value"""
    a = acc.reshape(acc.shape[:-1] + (4, 64))
    for m in (32, 16, 8, 4, 2, 1):
        a = a + a[..., _LANE ^ m]
    w = a[..., 0]
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def partials(u, v):
    """partial[0 .. G) of dot(u, v)"""
    n = len(u)
    G = grid(n)
    with np.errstate(all="ignore"):
        prod = np.asarray(u).astype(np.float64) * np.asarray(v).astype(np.float64)
        nchunks = -(-n // CHUNK)
        rounds = max(1, -(-nchunks // G))
        P = np.zeros(rounds * G * CHUNK, np.float64)
        P[:n] = prod
        P = P.reshape(rounds, G, PER, THREADS)
        acc = np.zeros((G, THREADS), np.float64)
        for rd in range(rounds):
            for j in range(PER):
                acc = acc + P[rd, :, j, :]
        return _tree(acc)


def total(partial):
    P = np.zeros(MAXG, np.float64)
    P[:len(partial)] = partial
    P = P.reshape(4, THREADS)
    with np.errstate(all="ignore"):
        acc = np.zeros(THREADS, np.float64)
        for j in range(4):
            acc = acc + P[j]
        return np.float64(_tree(acc))


def dot(u, v):
    return total(partials(u, v))


def solve(n, rp, ci, v, b, x0, method="cg", precond="none", minv=None, factor=None, max_iters=200, rtol=1e-8, atol=0.0,
          dtype=np.float64, oracle=None):
    """dict(x, iters, status, history, bb, rr, threshold, stop_iter, reason).  factor: (rp, ci, values) of the LU factor.  history
    holds the entries the solver writes (iters + 1 of them); stop_iter is the iteration during which the status was set (0: the
    start); reason names the test that set it."""
    dtype = np.dtype(dtype).type
    f8 = np.float64
    b = np.asarray(b, dtype)
    x = np.asarray(x0, dtype).copy()
    if minv is not None:
        minv = np.asarray(minv, dtype)

    def A(w):
        return mxvref.mxv(n, n, rp, ci, v, w, "plus_times", dtype, oracle=oracle)

    def M(r):
        if precond == "none":
            return r
        if precond == "diag":
            return minv * r
        frp, fci, fv = factor
        w = trsvref.trsv(n, frp, fci, fv, r, "lower", True, dtype)
        return trsvref.trsv(n, frp, fci, fv, w, "upper", False, dtype)

    hist = []
    out = dict(stop_iter=0, reason="")

    def done(status, iters, rr, k, reason):
        out.update(x=x, iters=iters, status=status, history=np.array(hist, f8), bb=bb, rr=rr, threshold=thr, stop_iter=k, reason=reason)
        return out

    def check(rr, k):
        if not np.isfinite(rr):
            return NONFINITE
        if rr <= thr:
            return CONVERGED
        if k == max_iters:
            return MAX_ITERS
        return None

    with np.errstate(all="ignore"):
        r = b - A(x)
        bb, rr = dot(b, b), dot(r, r)
        t1, t2 = (f8(rtol) * f8(rtol)) * bb, f8(atol) * f8(atol)
        thr = t1 if t1 > t2 else t2
        hist.append(rr)
        st = check(rr, 0)
        if st is not None:
            return done(st, 0, rr, 0, "check")
        if method == "cg":
            z = M(r)
            rz = dot(r, z)
            p = z.copy()
            k = 0
            while True:
                k += 1
                q = A(p)
                pq = dot(p, q)
                if not (pq > 0) or not np.isfinite(pq):
                    return done(BREAKDOWN, k - 1, rr, k, "pq")
                alpha = rz / pq
                av = dtype(alpha)
                x = x + av * p
                r = r - av * q
                z = M(r)
                rr, rzn = dot(r, r), dot(r, z)
                hist.append(rr)
                st = check(rr, k)
                if st is not None:
                    return done(st, k, rr, k, "check")
                beta = rzn / rz
                p = z + dtype(beta) * p
                rz = rzn
        # BiCGStab
        rhat = r.copy()
        rhon = rr
        if rhon == 0 or not np.isfinite(rhon):
            return done(BREAKDOWN, 0, rr, 0, "rho")
        p = r.copy()
        k = 0
        while True:
            k += 1
            y = M(p)
            vv = A(y)
            rv = dot(rhat, vv)
            if rv == 0 or not np.isfinite(rv):
                return done(BREAKDOWN, k - 1, rr, k, "rv")
            alpha = rhon / rv
            av = dtype(alpha)
            s = r - av * vv
            ss = dot(s, s)
            if ss <= thr:
                x = x + av * y
                hist.append(ss)
                return done(CONVERGED, k, ss, k, "ss")
            z = M(s)
            t = A(z)
            ts, tt = dot(t, s), dot(t, t)
            if not (tt > 0) or not np.isfinite(tt):
                return done(BREAKDOWN, k - 1, rr, k, "tt")
            omega = ts / tt
            ov = dtype(omega)
            x = (x + av * y) + ov * z
            r = s - ov * t
            rr = dot(r, r)
            rho = rhon
            rhon = dot(rhat, r)
            hist.append(rr)
            st = check(rr, k)
            if st is not None:
                return done(st, k, rr, k, "check")
            if omega == 0:
                return done(BREAKDOWN, k, rr, k, "omega")
            if rhon == 0 or not np.isfinite(rhon):
                return done(BREAKDOWN, k, rr, k, "rho")
            beta = (rhon / rho) * (alpha / omega)
            p = r + dtype(beta) * (p - ov * vv)


def readbacks(stop_iter, check_every):
    return max(1, -(-stop_iter // check_every))


def launches(method, precond, stop_iter, check_every, max_iters, trsv_launches=0):
    """res->launches by the header's formula: S + E * I"""
    E = min(max_iters, check_every * readbacks(stop_iter, check_every))
    T = trsv_launches if precond == "lu" else 0
    if method == "cg":
        S, I = (4 + T, 5 + T) if precond == "lu" else (3, 4)
    else:
        S, I = 3, 7 + 2 * T
    return S + E * I
