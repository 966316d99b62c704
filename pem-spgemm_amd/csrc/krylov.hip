// krylov.hip -- preconditioned CG and BiCGStab on a tiling (include/pem_spgemm.h, pem_krylov_*): A x = b solved on the context's
// stream, the preconditioner none, a diagonal, an LU factor (two pem_tiled_trsv per application) or a multigrid hierarchy (one
// pem_amg_apply per application, where LU runs its solves: the [LU: ...] launches below with T = pem_amg_info::launches).
//
// The order is the contract; the header states it in full.  What this file adds to it is the launch structure:
//   Every vector kernel runs the SAME partition of [0, n): chunks of KR_CHUNK = 4096 elements, G = min(ceil(n / 4096), 1024)
//   workgroups of 256 threads, workgroup g the chunks g, g + G, ..., thread t the elements chunk * 4096 + t + 256 j, j = 0 .. 15.
//   A dot product is one fp64 chain acc = acc + u_i * v_i per thread in ascending i, the xor butterfly 32 .. 1 over the wave's 64
//   lanes, (w0 + w1) + (w2 + w3) over the four waves: partial[g].  No kernel finishes a dot it started: the kernel AFTER it sums
//   the G partials in its prologue -- thread t takes partial[t], [t + 256], [t + 512], [t + 768] in that order, then the same tree --
//   in every workgroup alike, so every workgroup derives the same scalar bits and takes the same branch.  No floating-point
//   atomics, nothing waits on another workgroup, no kernel reads what the same launch writes: the state block (KState) is read
//   from one copy and written, by workgroup 0 alone, to the other; the host alternates the two.  Every dot has partial slots of
//   its own, and the kernel that writes a slot never reads it.
//   Once the state's status is set every later solver kernel returns in its prologue (workgroup 0 copies the state on), so x, r, p
//   and d_history stay as they were; the mxv and trsv launches in between write scratch vectors only.
//
// Launches (solver kernels by their kernel_stats names; T = the trsv launches of both triangles of F):
//   CG        start      mxv, krylov_init, [LU: T, krylov_dot], krylov_cg_p
//             iteration  mxv, krylov_dot (pq), krylov_cg_update, [LU: T, krylov_dot (rz')], krylov_cg_p
//   BiCGStab  start      mxv, krylov_init, krylov_bi_p
//             iteration  [LU: T] mxv, krylov_dot (rv), krylov_bi_s, [LU: T] mxv, krylov_bi_ts, krylov_bi_xr, krylov_bi_p
#include "spgemm_internal.h"
#include "tiled_internal.h"
#include "mx_internal.h"

using namespace pem;

namespace {

constexpr int KR_THREADS = 256;
constexpr int KR_PER = 16;                        // elements per thread and chunk
constexpr int KR_CHUNK = KR_THREADS * KR_PER;     // 4096
constexpr int KR_MAXG = 1024;                     // workgroups, and partials per slot
constexpr long long KR_RUNNING = -1;              // KState::status while no pem_krylov status is set

// the state block: 16 eight-byte words, read back in one copy
struct KState {
    long long iters, status;
    double bb, rr, threshold;
    double rz;      // CG: dot(r, z) of the current z
    double rho;     // BiCGStab: the current rho' = dot(rhat, r)
    double alpha, omega;
    long long pad[7];
};
static_assert(sizeof(KState) == 128, "the state block is 16 words");

__device__ __forceinline__ bool kr_finite(double v) { return __builtin_isfinite(v); }

// the block tree: butterfly inside the wave, (w0 + w1) + (w2 + w3) across; every thread gets the result
__device__ __forceinline__ double kr_tree(double acc, double *s4)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc = acc + __shfl_xor(acc, m, 64);
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = acc;
    __syncthreads();
    const double t = (s4[0] + s4[1]) + (s4[2] + s4[3]);
    __syncthreads();
    return t;
}

__device__ __forceinline__ double kr_total(const double *__restrict__ partial, int G, double *s4)
{
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = (int)threadIdx.x + KR_THREADS * j;
        if (i < G) acc = acc + partial[i];
    }
    return kr_tree(acc, s4);
}

// f(i) for this thread's elements in ascending i
template <typename F>
__device__ __forceinline__ void kr_for(const long long n, F f)
{
    const long long nchunks = (n + KR_CHUNK - 1) / KR_CHUNK;
    for (long long c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const long long base = c * KR_CHUNK + threadIdx.x;
        if (c * KR_CHUNK + KR_CHUNK <= n) {
#pragma unroll
            for (int j = 0; j < KR_PER; ++j) f(base + KR_THREADS * j);
        } else {
#pragma unroll
            for (int j = 0; j < KR_PER; ++j) {
                const long long i = base + KR_THREADS * j;
                if (i < n) f(i);
            }
        }
    }
}

__device__ __forceinline__ void kr_put(double *partial, double acc, double *s4)
{
    const double t = kr_tree(acc, s4);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

__device__ __forceinline__ void kr_pass(const KState &S, KState *out)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) *out = S;
}

template <typename VT> __device__ __forceinline__ double kr_prod(VT a, VT b) { return (double)a * (double)b; }

// z_i of the on-the-fly preconditioners (NONE: r_i; DIAG: minv_i * r_i); LU reads its z from an array
template <typename VT, int PC> __device__ __forceinline__ VT kr_z(const VT ri, const VT *minv, const VT *zarr, long long i)
{
    if constexpr (PC == PEM_PRECOND_NONE) return ri;
    else if constexpr (PC == PEM_PRECOND_DIAG) return minv[i] * ri;
    else return zarr[i];
}

// partial[g] of dot(u, v); in: the state (null: run whatever it says -- the start of a solve, the test hook)
template <typename VT>
__global__ void __launch_bounds__(KR_THREADS) kr_dot_kernel(const long long n, const KState *__restrict__ in, const VT *__restrict__ u,
                                                            const VT *__restrict__ v, double *__restrict__ partial)
{
    __shared__ double s4[4];
    if (in && in->status != KR_RUNNING) return;
    double acc = 0.0;
    kr_for(n, [&](long long i) { acc = acc + kr_prod(u[i], v[i]); });
    kr_put(partial, acc, s4);
}

// the hook's total: one workgroup
__global__ void __launch_bounds__(KR_THREADS) kr_total_kernel(const double *__restrict__ partial, const int G, double *__restrict__ out)
{
    __shared__ double s4[4];
    const double t = kr_total(partial, G, s4);
    if (threadIdx.x == 0) *out = t;
}

// r = b - q, the partials of bb, rr and (CG, not LU) rz
template <typename VT, int PC, bool CG>
__global__ void __launch_bounds__(KR_THREADS) kr_init_kernel(const long long n, const VT *__restrict__ b, const VT *__restrict__ q, VT *__restrict__ r,
                                                             const VT *__restrict__ minv, double *__restrict__ pbb, double *__restrict__ prr,
                                                             double *__restrict__ prz)
{
    __shared__ double s4[4];
    double abb = 0.0, arr = 0.0, arz = 0.0;
    kr_for(n, [&](long long i) {
        const VT bi = b[i];
        const VT ri = bi - q[i];
        r[i] = ri;
        abb = abb + kr_prod(bi, bi);
        arr = arr + kr_prod(ri, ri);
        if constexpr (CG && PC != PEM_PRECOND_LU) arz = arz + kr_prod(ri, kr_z<VT, PC>(ri, minv, nullptr, i));
    });
    kr_put(pbb, abb, s4);
    kr_put(prr, arr, s4);
    if constexpr (CG && PC != PEM_PRECOND_LU) kr_put(prz, arz, s4);
}

// the start of a solve, shared: bb, rr, the threshold, history[0].  Returns the state every thread holds.
__device__ __forceinline__ KState kr_start(const double *pbb, const double *prr, int G, double rtol, double atol, double *history, double *s4)
{
    KState S = {};
    S.bb = kr_total(pbb, G, s4);
    S.rr = kr_total(prr, G, s4);
    const double t1 = (rtol * rtol) * S.bb, t2 = atol * atol;
    S.threshold = t1 > t2 ? t1 : t2;
    S.iters = 0;
    S.status = KR_RUNNING;
    if (history && blockIdx.x == 0 && threadIdx.x == 0) history[0] = S.rr;
    return S;
}

// NONFINITE / CONVERGED / MAX_ITERS on S.rr at iteration S.iters
__device__ __forceinline__ void kr_check(KState &S, long long max_iters)
{
    if (!kr_finite(S.rr)) S.status = PEM_KRYLOV_NONFINITE;
    else if (S.rr <= S.threshold) S.status = PEM_KRYLOV_CONVERGED;
    else if (S.iters == max_iters) S.status = PEM_KRYLOV_MAX_ITERS;
}

// CG: the end of iteration k (FIRST: of the start): the totals of rr and rz', history[k], the checks, beta, p = z + beta p
template <typename VT, int PC, bool FIRST>
__global__ void __launch_bounds__(KR_THREADS) cg_p_kernel(const long long n, const KState *__restrict__ in, KState *__restrict__ out,
                                                          const double *__restrict__ pbb, const double *__restrict__ prr,
                                                          const double *__restrict__ prz, const int G, const VT *__restrict__ r,
                                                          const VT *__restrict__ zarr, const VT *__restrict__ minv, VT *__restrict__ p,
                                                          double *__restrict__ history, const long long max_iters, const double rtol, const double atol)
{
    __shared__ double s4[4];
    KState S;
    double beta = 0.0;
    if constexpr (FIRST) {
        S = kr_start(pbb, prr, G, rtol, atol, history, s4);
        S.rz = kr_total(prz, G, s4);
    } else {
        S = *in;
        if (S.status != KR_RUNNING) {
            kr_pass(S, out);
            return;
        }
        S.rr = kr_total(prr, G, s4);
        const double rzn = kr_total(prz, G, s4);
        S.iters += 1;
        if (history && blockIdx.x == 0 && threadIdx.x == 0) history[S.iters] = S.rr;
        beta = rzn / S.rz;
        S.rz = rzn;
    }
    kr_check(S, max_iters);
    kr_pass(S, out);
    if (S.status != KR_RUNNING) return;
    const VT bv = (VT)beta;
    kr_for(n, [&](long long i) {
        const VT zi = kr_z<VT, PC>(r[i], minv, zarr, i);
        if constexpr (FIRST) p[i] = zi;
        else {
            const VT t = bv * p[i];
            p[i] = zi + t;
        }
    });
}

// CG: pq's total, the breakdown check, alpha, x += alpha p, r -= alpha q, the partials of rr and (not LU) rz'
template <typename VT, int PC>
__global__ void __launch_bounds__(KR_THREADS) cg_update_kernel(const long long n, const KState *__restrict__ in, KState *__restrict__ out,
                                                               const double *__restrict__ ppq, const int G, VT *__restrict__ x, VT *__restrict__ r,
                                                               const VT *__restrict__ p, const VT *__restrict__ q, const VT *__restrict__ minv,
                                                               double *__restrict__ prr, double *__restrict__ prz)
{
    __shared__ double s4[4];
    KState S = *in;
    if (S.status != KR_RUNNING) {
        kr_pass(S, out);
        return;
    }
    const double pq = kr_total(ppq, G, s4);
    if (!(pq > 0.0) || !kr_finite(pq)) {
        S.status = PEM_KRYLOV_BREAKDOWN;
        kr_pass(S, out);
        return;
    }
    S.alpha = S.rz / pq;
    kr_pass(S, out);
    const VT av = (VT)S.alpha;
    double arr = 0.0, arz = 0.0;
    kr_for(n, [&](long long i) {
        const VT t1 = av * p[i];
        x[i] = x[i] + t1;
        const VT t2 = av * q[i];
        const VT ri = r[i] - t2;
        r[i] = ri;
        arr = arr + kr_prod(ri, ri);
        if constexpr (PC != PEM_PRECOND_LU) arz = arz + kr_prod(ri, kr_z<VT, PC>(ri, minv, nullptr, i));
    });
    kr_put(prr, arr, s4);
    if constexpr (PC != PEM_PRECOND_LU) kr_put(prz, arz, s4);
}

// BiCGStab: the end of iteration k and the head of k + 1 (FIRST: the start and the head of 1)
template <typename VT, int PC, bool FIRST>
__global__ void __launch_bounds__(KR_THREADS) bi_p_kernel(const long long n, const KState *__restrict__ in, KState *__restrict__ out,
                                                          const double *__restrict__ pbb, const double *__restrict__ prr,
                                                          const double *__restrict__ prho, const int G, const VT *__restrict__ r,
                                                          VT *__restrict__ rhat, VT *__restrict__ p, const VT *__restrict__ v, VT *__restrict__ y,
                                                          const VT *__restrict__ minv, double *__restrict__ history, const long long max_iters,
                                                          const double rtol, const double atol)
{
    __shared__ double s4[4];
    KState S;
    double rhon, beta = 0.0;
    if constexpr (FIRST) {
        S = kr_start(pbb, prr, G, rtol, atol, history, s4);
        rhon = S.rr;
    } else {
        S = *in;
        if (S.status != KR_RUNNING) {
            kr_pass(S, out);
            return;
        }
        S.rr = kr_total(prr, G, s4);
        rhon = kr_total(prho, G, s4);
        S.iters += 1;
        if (history && blockIdx.x == 0 && threadIdx.x == 0) history[S.iters] = S.rr;
    }
    kr_check(S, max_iters);
    if (S.status == KR_RUNNING) {
        if (!FIRST && S.omega == 0.0) S.status = PEM_KRYLOV_BREAKDOWN;
        else if (rhon == 0.0 || !kr_finite(rhon)) S.status = PEM_KRYLOV_BREAKDOWN;
    }
    if (S.status == KR_RUNNING) {
        if (!FIRST) beta = (rhon / S.rho) * (S.alpha / S.omega);
        S.rho = rhon;
    }
    kr_pass(S, out);
    if (S.status != KR_RUNNING) return;
    const VT bv = (VT)beta, ov = (VT)S.omega;
    kr_for(n, [&](long long i) {
        const VT ri = r[i];
        VT pi;
        if constexpr (FIRST) {
            rhat[i] = ri;
            pi = ri;
        } else {
            const VT t1 = ov * v[i];
            const VT t2 = p[i] - t1;
            const VT t3 = bv * t2;
            pi = ri + t3;
        }
        p[i] = pi;
        if constexpr (PC == PEM_PRECOND_DIAG) y[i] = minv[i] * pi;
    });
}

// BiCGStab: rv's total, its check, alpha, s = r - alpha v, the partial of ss (DIAG: z = minv s)
template <typename VT, int PC>
__global__ void __launch_bounds__(KR_THREADS) bi_s_kernel(const long long n, const KState *__restrict__ in, KState *__restrict__ out,
                                                          const double *__restrict__ prv, const int G, const VT *__restrict__ r,
                                                          const VT *__restrict__ v, VT *__restrict__ s, VT *__restrict__ z,
                                                          const VT *__restrict__ minv, double *__restrict__ pss)
{
    __shared__ double s4[4];
    KState S = *in;
    if (S.status != KR_RUNNING) {
        kr_pass(S, out);
        return;
    }
    const double rv = kr_total(prv, G, s4);
    if (rv == 0.0 || !kr_finite(rv)) {
        S.status = PEM_KRYLOV_BREAKDOWN;
        kr_pass(S, out);
        return;
    }
    S.alpha = S.rho / rv;
    kr_pass(S, out);
    const VT av = (VT)S.alpha;
    double ass = 0.0;
    kr_for(n, [&](long long i) {
        const VT t = av * v[i];
        const VT si = r[i] - t;
        s[i] = si;
        ass = ass + kr_prod(si, si);
        if constexpr (PC == PEM_PRECOND_DIAG) z[i] = minv[i] * si;
    });
    kr_put(pss, ass, s4);
}

// BiCGStab: ss's total; converged there: x += alpha y and the end; else the partials of ts and tt
template <typename VT>
__global__ void __launch_bounds__(KR_THREADS) bi_ts_kernel(const long long n, const KState *__restrict__ in, KState *__restrict__ out,
                                                           const double *__restrict__ pss, const int G, VT *__restrict__ x, const VT *__restrict__ y,
                                                           const VT *__restrict__ s, const VT *__restrict__ t, double *__restrict__ history,
                                                           double *__restrict__ pts, double *__restrict__ ptt)
{
    __shared__ double s4[4];
    KState S = *in;
    if (S.status != KR_RUNNING) {
        kr_pass(S, out);
        return;
    }
    const double ss = kr_total(pss, G, s4);
    if (ss <= S.threshold) {
        S.iters += 1;
        S.rr = ss;
        S.status = PEM_KRYLOV_CONVERGED;
        if (history && blockIdx.x == 0 && threadIdx.x == 0) history[S.iters] = ss;
        kr_pass(S, out);
        const VT av = (VT)S.alpha;
        kr_for(n, [&](long long i) {
            const VT t1 = av * y[i];
            x[i] = x[i] + t1;
        });
        return;
    }
    kr_pass(S, out);
    double ats = 0.0, att = 0.0;
    kr_for(n, [&](long long i) {
        const VT ti = t[i];
        ats = ats + kr_prod(ti, s[i]);
        att = att + kr_prod(ti, ti);
    });
    kr_put(pts, ats, s4);
    kr_put(ptt, att, s4);
}

// BiCGStab: the totals of ts and tt, the check, omega, x = (x + alpha y) + omega z, r = s - omega t, the partials of rr and rho'
template <typename VT>
__global__ void __launch_bounds__(KR_THREADS) bi_xr_kernel(const long long n, const KState *__restrict__ in, KState *__restrict__ out,
                                                           const double *__restrict__ pts, const double *__restrict__ ptt, const int G,
                                                           VT *__restrict__ x, const VT *__restrict__ y, const VT *__restrict__ z,
                                                           const VT *__restrict__ s, const VT *__restrict__ t, VT *__restrict__ r,
                                                           const VT *__restrict__ rhat, double *__restrict__ prr, double *__restrict__ prho)
{
    __shared__ double s4[4];
    KState S = *in;
    if (S.status != KR_RUNNING) {
        kr_pass(S, out);
        return;
    }
    const double ts = kr_total(pts, G, s4);
    const double tt = kr_total(ptt, G, s4);
    if (!(tt > 0.0) || !kr_finite(tt)) {
        S.status = PEM_KRYLOV_BREAKDOWN;
        kr_pass(S, out);
        return;
    }
    S.omega = ts / tt;
    kr_pass(S, out);
    const VT av = (VT)S.alpha, ov = (VT)S.omega;
    double arr = 0.0, arho = 0.0;
    kr_for(n, [&](long long i) {
        const VT t1 = av * y[i];
        const VT xa = x[i] + t1;
        const VT t2 = ov * z[i];
        x[i] = xa + t2;
        const VT t3 = ov * t[i];
        const VT ri = s[i] - t3;
        r[i] = ri;
        arr = arr + kr_prod(ri, ri);
        arho = arho + kr_prod(rhat[i], ri);
    });
    kr_put(prr, arr, s4);
    kr_put(prho, arho, s4);
}

int kr_grid(int64_t n)
{
    const int64_t c = (n + KR_CHUNK - 1) / KR_CHUNK;
    return (int)(c < 1 ? 1 : (c > KR_MAXG ? KR_MAXG : c));
}

// the partial slots, one per dot that is in flight: bb; rr; rz' (BiCGStab: rho'); pq (rv); ss; ts; tt
enum { SLOT_BB = 0, SLOT_RR, SLOT_RZ, SLOT_A, SLOT_B, SLOT_C, SLOT_D, KR_SLOTS };

}  // namespace

struct pem_krylov {
    pem_ctx *owner = nullptr;
    const pem_tiled *A = nullptr, *F = nullptr;
    const pem_amg *M = nullptr;  // PEM_PRECOND_AMG: z = one V-cycle, on the LU path
    pem_krylov_opts opts = {};
    DevBuf buf;                 // the work vectors, the partial slots, the two state blocks
    void *vec[9] = {};          // CG: r p q z w;  BiCGStab: r rhat p v s t y z w
    double *slot[8] = {};
    KState *state[2] = {};
    int seq = 0;                // state[seq & 1] is the current one
    int64_t launches = 0;
};

namespace {

template <typename VT>
struct Run {
    pem_ctx *ctx;
    pem_krylov *K;
    long long n;
    int G;
    const VT *b, *minv;
    VT *x;
    double *history;
    int64_t trsv_launches;

    VT *v(int i) const { return (VT *)K->vec[i]; }
    const KState *in() const { return K->state[K->seq & 1]; }
    KState *out() const { return K->state[(K->seq + 1) & 1]; }
    void flip()
    {
        ++K->seq;
        ++K->launches;
    }

    pem_status mxv(const VT *xin, VT *y)
    {
        ++K->launches;
        return mxv_semiring(ctx, K->A, PEM_SEMIRING_PLUS_TIMES, false, xin, y, 0);
    }
    // dst = U^-1 L^-1 src through the work vector w; with a hierarchy dst = one V-cycle on src (w is not carved)
    pem_status lu(const VT *src, VT *w, VT *dst)
    {
        K->launches += trsv_launches;
        if (K->M) {
            pem_amg *M = const_cast<pem_amg *>(K->M);
            if constexpr (sizeof(VT) == 8) return pem_amg_apply(ctx, M, src, dst);
            else return pem_amg_apply_f32(ctx, M, src, dst);
        }
        if constexpr (sizeof(VT) == 8) {
            PEM_TRY(pem_tiled_trsv(ctx, K->F, PEM_TRSV_LOWER, 1, src, w));
            return pem_tiled_trsv(ctx, K->F, PEM_TRSV_UPPER, 0, w, dst);
        } else {
            PEM_TRY(pem_tiled_trsv_f32(ctx, K->F, PEM_TRSV_LOWER, 1, src, w));
            return pem_tiled_trsv_f32(ctx, K->F, PEM_TRSV_UPPER, 0, w, dst);
        }
    }
    void dot(const KState *st, const VT *u, const VT *w, double *partial)
    {
        PEM_LAUNCH_NAMED(ctx, "krylov_dot", (kr_dot_kernel<VT>), G, KR_THREADS, n, st, u, w, partial);
        ++K->launches;
    }

    // ---- CG: vec = r p q z w ----
    template <int PC> pem_status cg_start()
    {
        const pem_krylov_opts &o = K->opts;
        double **s = K->slot;
        PEM_TRY(mxv(x, v(2)));
        PEM_LAUNCH_NAMED(ctx, "krylov_init", (kr_init_kernel<VT, PC, true>), G, KR_THREADS, n, b, (const VT *)v(2), v(0), minv, s[SLOT_BB], s[SLOT_RR],
                         s[SLOT_RZ]);
        ++K->launches;
        if (PC == PEM_PRECOND_LU) {
            PEM_TRY(lu(v(0), v(4), v(3)));
            dot(nullptr, v(0), v(3), s[SLOT_RZ]);
        }
        PEM_LAUNCH_NAMED(ctx, "krylov_cg_p", (cg_p_kernel<VT, PC, true>), G, KR_THREADS, n, (const KState *)nullptr, out(), s[SLOT_BB], s[SLOT_RR],
                         s[SLOT_RZ], G, (const VT *)v(0), (const VT *)v(3), minv, v(1), history, (long long)o.max_iters, o.rtol, o.atol);
        flip();
        return PEM_OK;
    }
    template <int PC> pem_status cg_iter()
    {
        const pem_krylov_opts &o = K->opts;
        double **s = K->slot;
        PEM_TRY(mxv(v(1), v(2)));
        dot(in(), v(1), v(2), s[SLOT_A]);
        PEM_LAUNCH_NAMED(ctx, "krylov_cg_update", (cg_update_kernel<VT, PC>), G, KR_THREADS, n, in(), out(), s[SLOT_A], G, x, v(0), (const VT *)v(1),
                         (const VT *)v(2), minv, s[SLOT_RR], s[SLOT_RZ]);
        flip();
        if (PC == PEM_PRECOND_LU) {
            PEM_TRY(lu(v(0), v(4), v(3)));
            dot(in(), v(0), v(3), s[SLOT_RZ]);
        }
        PEM_LAUNCH_NAMED(ctx, "krylov_cg_p", (cg_p_kernel<VT, PC, false>), G, KR_THREADS, n, in(), out(), s[SLOT_BB], s[SLOT_RR], s[SLOT_RZ], G,
                         (const VT *)v(0), (const VT *)v(3), minv, v(1), history, (long long)o.max_iters, o.rtol, o.atol);
        flip();
        return PEM_OK;
    }

    // ---- BiCGStab: vec = r rhat p v s t y z w; without a preconditioner y is p and z is s ----
    template <int PC> VT *yv() const { return PC == PEM_PRECOND_NONE ? v(2) : v(6); }
    template <int PC> VT *zv() const { return PC == PEM_PRECOND_NONE ? v(4) : v(7); }
    template <int PC> pem_status bi_start()
    {
        const pem_krylov_opts &o = K->opts;
        double **s = K->slot;
        PEM_TRY(mxv(x, v(3)));
        PEM_LAUNCH_NAMED(ctx, "krylov_init", (kr_init_kernel<VT, PC, false>), G, KR_THREADS, n, b, (const VT *)v(3), v(0), minv, s[SLOT_BB],
                         s[SLOT_RR], s[SLOT_RZ]);
        ++K->launches;
        PEM_LAUNCH_NAMED(ctx, "krylov_bi_p", (bi_p_kernel<VT, PC, true>), G, KR_THREADS, n, (const KState *)nullptr, out(), s[SLOT_BB], s[SLOT_RR],
                         s[SLOT_RZ], G, (const VT *)v(0), v(1), v(2), (const VT *)v(3), yv<PC>(), minv, history, (long long)o.max_iters, o.rtol,
                         o.atol);
        flip();
        return PEM_OK;
    }
    template <int PC> pem_status bi_iter()
    {
        const pem_krylov_opts &o = K->opts;
        double **s = K->slot;
        VT *y = yv<PC>(), *z = zv<PC>();
        if (PC == PEM_PRECOND_LU) PEM_TRY(lu(v(2), v(8), y));
        PEM_TRY(mxv(y, v(3)));
        dot(in(), v(1), v(3), s[SLOT_A]);
        PEM_LAUNCH_NAMED(ctx, "krylov_bi_s", (bi_s_kernel<VT, PC>), G, KR_THREADS, n, in(), out(), s[SLOT_A], G, (const VT *)v(0), (const VT *)v(3),
                         v(4), v(7), minv, s[SLOT_B]);
        flip();
        if (PC == PEM_PRECOND_LU) PEM_TRY(lu(v(4), v(8), z));
        PEM_TRY(mxv(z, v(5)));
        PEM_LAUNCH_NAMED(ctx, "krylov_bi_ts", (bi_ts_kernel<VT>), G, KR_THREADS, n, in(), out(), s[SLOT_B], G, x, (const VT *)y, (const VT *)v(4),
                         (const VT *)v(5), history, s[SLOT_C], s[SLOT_D]);
        flip();
        PEM_LAUNCH_NAMED(ctx, "krylov_bi_xr", (bi_xr_kernel<VT>), G, KR_THREADS, n, in(), out(), s[SLOT_C], s[SLOT_D], G, x, (const VT *)y,
                         (const VT *)z, (const VT *)v(4), (const VT *)v(5), v(0), (const VT *)v(1), s[SLOT_RR], s[SLOT_RZ]);
        flip();
        PEM_LAUNCH_NAMED(ctx, "krylov_bi_p", (bi_p_kernel<VT, PC, false>), G, KR_THREADS, n, in(), out(), s[SLOT_BB], s[SLOT_RR], s[SLOT_RZ], G,
                         (const VT *)v(0), v(1), v(2), (const VT *)v(3), y, minv, history, (long long)o.max_iters, o.rtol, o.atol);
        flip();
        return PEM_OK;
    }

    template <int PC> pem_status start() { return K->opts.method == PEM_KRYLOV_CG ? cg_start<PC>() : bi_start<PC>(); }
    template <int PC> pem_status iter() { return K->opts.method == PEM_KRYLOV_CG ? cg_iter<PC>() : bi_iter<PC>(); }
    pem_status start()
    {
        switch (K->opts.precond) {
        case PEM_PRECOND_NONE: return start<PEM_PRECOND_NONE>();
        case PEM_PRECOND_DIAG: return start<PEM_PRECOND_DIAG>();
        default: return start<PEM_PRECOND_LU>();
        }
    }
    pem_status iter()
    {
        switch (K->opts.precond) {
        case PEM_PRECOND_NONE: return iter<PEM_PRECOND_NONE>();
        case PEM_PRECOND_DIAG: return iter<PEM_PRECOND_DIAG>();
        default: return iter<PEM_PRECOND_LU>();
        }
    }
};

template <typename VT>
pem_status krylov_run(pem_ctx *ctx, pem_krylov *K, const VT *b, VT *x, const VT *minv, double *history, pem_krylov_result *res)
{
    Run<VT> R{ctx, K, (long long)K->A->rows, kr_grid(K->A->rows), b, minv, x, history, 0};
    if (K->opts.precond == PEM_PRECOND_LU) {
        pem_trsv_info lo, up;
        PEM_TRY(pem_tiled_trsv_info(ctx, K->F, PEM_TRSV_LOWER, &lo));
        PEM_TRY(pem_tiled_trsv_info(ctx, K->F, PEM_TRSV_UPPER, &up));
        R.trsv_launches = lo.launches + up.launches;
    }
    if (K->M) {
        pem_amg_info mi;
        PEM_TRY(pem_amg_get_info(K->M, &mi));
        R.trsv_launches = mi.launches;
    }
    K->launches = 0;
    PEM_TRY(R.start());
    KState S;
    int64_t enqueued = 0, readbacks = 0;
    for (;;) {
        const int64_t left = K->opts.max_iters - enqueued;
        const int64_t batch = left < K->opts.check_every ? left : K->opts.check_every;
        for (int64_t i = 0; i < batch; ++i) PEM_TRY(R.iter());
        enqueued += batch;
        PEM_TRY(read_scalars(ctx, reinterpret_cast<const int64_t *>(R.in()), (int)(sizeof(KState) / 8), reinterpret_cast<int64_t *>(&S)));
        PEM_TRY(launch_status(ctx));
        ++readbacks;
        if (S.status != KR_RUNNING) break;
        if (enqueued >= K->opts.max_iters) {
            set_error("pem_krylov_solve: internal: %lld iterations ran and no status is set", (long long)enqueued);
            return PEM_E_HIP;
        }
    }
    res->iters = S.iters;
    res->status = (int)S.status;
    res->bb = S.bb;
    res->rr = S.rr;
    res->threshold = S.threshold;
    res->readbacks = readbacks;
    res->launches = K->launches;
    return PEM_OK;
}

bool kr_bad_tol(double t) { return !(t >= 0.0); }   // negative or NaN

pem_status krylov_solve(pem_ctx *ctx, pem_krylov *K, const void *db, void *dx, const void *dminv, double *dhist, pem_krylov_result *res,
                        int value_bytes, const char *fn)
{
    if (!ctx || !K) {
        set_error("%s: null context or solver", fn);
        return PEM_E_INVALID;
    }
    if (K->owner != ctx) {
        set_error("%s: the solver was created on another context", fn);
        return PEM_E_INVALID;
    }
    if (K->A->value_bytes != value_bytes) {
        set_error("%s: the tiling holds %s values; use the %s entry point", fn, K->A->value_bytes == 4 ? "fp32" : "fp64",
                  K->A->value_bytes == 4 ? "_f32" : "fp64");
        return PEM_E_INVALID;
    }
    if (!res) {
        set_error("%s: null res", fn);
        return PEM_E_INVALID;
    }
    const size_t n = (size_t)K->A->rows;
    const pem_krylov_opts &o = K->opts;
    if (n == 0) {
        *res = pem_krylov_result{};
        res->status = PEM_KRYLOV_CONVERGED;
        res->threshold = o.atol * o.atol;
        return PEM_OK;
    }
    if (!db || !dx) {
        set_error("%s: null vector", fn);
        return PEM_E_INVALID;
    }
    if (o.precond == PEM_PRECOND_DIAG && !dminv) {
        set_error("%s: the solver was created with PEM_PRECOND_DIAG; d_minv is null", fn);
        return PEM_E_INVALID;
    }
    if (o.precond != PEM_PRECOND_DIAG) dminv = nullptr;
    const Span sp[4] = {Span(db, n * value_bytes), Span(dx, n * value_bytes), Span(dminv, n * value_bytes),
                        Span(dhist, ((size_t)o.max_iters + 1) * sizeof(double))};
    static const char *const names[4] = {"db", "dx", "d_minv", "d_history"};
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j)
            if (sp[i].meets(sp[j])) {
                set_error("%s: %s and %s overlap", fn, names[i], names[j]);
                return PEM_E_INVALID;
            }
    PEM_ENTER(ctx);
    if (value_bytes == 4) return krylov_run<float>(ctx, K, (const float *)db, (float *)dx, (const float *)dminv, dhist, res);
    return krylov_run<double>(ctx, K, (const double *)db, (double *)dx, (const double *)dminv, dhist, res);
}

}  // namespace

// pem_krylov_create (M null) and pem_krylov_create_amg (F null; amg: a hierarchy is expected)
static pem_status krylov_create(const char *fn, pem_ctx *ctx, const pem_tiled *A, const pem_krylov_opts *opts, const pem_tiled *F,
                                const pem_amg *M, bool amg, pem_krylov **out)
{
    if (out) *out = nullptr;
    if (!ctx || !A || !opts || !out || (amg && !M)) {
        set_error("%s: null argument", fn);
        return PEM_E_INVALID;
    }
    if (A->rows != A->cols) {
        set_error("%s: the tiling is %d x %d; a Krylov solver needs a square one", fn, A->rows, A->cols);
        return PEM_E_INVALID;
    }
    if (opts->method != PEM_KRYLOV_CG && opts->method != PEM_KRYLOV_BICGSTAB) {
        set_error("%s: unknown method %d (PEM_KRYLOV_CG = 0, PEM_KRYLOV_BICGSTAB = 1)", fn, opts->method);
        return PEM_E_INVALID;
    }
    if (amg) {
        if (opts->precond != PEM_PRECOND_AMG) {
            set_error("%s: the preconditioner must be PEM_PRECOND_AMG = 3 (got %d)", fn, opts->precond);
            return PEM_E_INVALID;
        }
        if (amg_owner(M) != ctx || amg_operator(M) != A) {
            set_error("%s: the hierarchy was created on another %s", fn, amg_owner(M) != ctx ? "context" : "tiling than A");
            return PEM_E_INVALID;
        }
    } else if (opts->precond < PEM_PRECOND_NONE || opts->precond > PEM_PRECOND_LU) {
        set_error("%s: unknown preconditioner %d (PEM_PRECOND_NONE, _DIAG, _LU = 0, 1, 2)", fn, opts->precond);
        return PEM_E_INVALID;
    }
    if (opts->precond == PEM_PRECOND_LU && !F) {
        set_error("%s: PEM_PRECOND_LU needs the factor F", fn);
        return PEM_E_INVALID;
    }
    if (opts->precond != PEM_PRECOND_LU && F) {
        set_error("%s: a factor F is given, but the preconditioner is not PEM_PRECOND_LU", fn);
        return PEM_E_INVALID;
    }
    if (F && (F->rows != A->rows || F->cols != A->cols || F->value_bytes != A->value_bytes)) {
        set_error("%s: F is %d x %d of %s, A is %d x %d of %s; the factor has A's size and value type", fn, F->rows, F->cols,
                  F->value_bytes == 4 ? "fp32" : "fp64", A->rows, A->cols, A->value_bytes == 4 ? "fp32" : "fp64");
        return PEM_E_INVALID;
    }
    if (opts->max_iters < 0 || opts->check_every < 1 || kr_bad_tol(opts->rtol) || kr_bad_tol(opts->atol)) {
        set_error("%s: max_iters >= 0, check_every >= 1, rtol >= 0 and atol >= 0 are required (got %lld, %lld, %g, %g)", fn,
                  (long long)opts->max_iters, (long long)opts->check_every, opts->rtol, opts->atol);
        return PEM_E_INVALID;
    }
    PEM_ENTER(ctx);
    const size_t n = (size_t)A->rows;
    if (F && n) {
        for (int uplo = 0; uplo < 2; ++uplo) {
            PEM_TRY(ensure_trsv(ctx, F, uplo));
            const TrsvSched &S = F->trsv[uplo];
            if (uplo == PEM_TRSV_UPPER && S.missing_diag) {
                set_error("%s: row %lld has no stored diagonal entry (%lld such rows); store it or pass unit_diag = 1", "pem_tiled_trsv",
                          (long long)S.first_missing_row, (long long)S.missing_diag);
                return PEM_E_INVALID;
            }
        }
    }
    std::unique_ptr<pem_krylov> K(new pem_krylov);
    K->owner = ctx;
    K->A = A;
    K->F = F;
    K->M = M;
    K->opts = *opts;
    const bool cg = opts->method == PEM_KRYLOV_CG;
    int nvec;
    if (amg) nvec = cg ? 4 : 8;   // LU's vectors without the trsv work vector w
    else if (cg) nvec = opts->precond == PEM_PRECOND_LU ? 5 : 3;
    else nvec = opts->precond == PEM_PRECOND_LU ? 9 : (opts->precond == PEM_PRECOND_DIAG ? 8 : 6);
    const size_t vbytes = (n * (size_t)A->value_bytes + 255) & ~size_t(255);
    const size_t sbytes = sizeof(double) * KR_MAXG;
    PEM_TRY(K->buf.reserve(vbytes * nvec + sbytes * KR_SLOTS + 2 * 256));
    char *p = K->buf.as<char>();
    for (int i = 0; i < nvec; ++i, p += vbytes) K->vec[i] = p;
    for (int i = 0; i < KR_SLOTS; ++i, p += sbytes) K->slot[i] = reinterpret_cast<double *>(p);
    for (int i = 0; i < 2; ++i, p += 256) K->state[i] = reinterpret_cast<KState *>(p);
    *out = K.release();
    return PEM_OK;
}

extern "C" pem_status pem_krylov_create(pem_ctx *ctx, const pem_tiled *A, const pem_krylov_opts *opts, const pem_tiled *F, pem_krylov **out)
{
    return krylov_create("pem_krylov_create", ctx, A, opts, F, nullptr, false, out);
}

extern "C" pem_status pem_krylov_create_amg(pem_ctx *ctx, const pem_tiled *A, const pem_krylov_opts *opts, const pem_amg *M, pem_krylov **out)
{
    return krylov_create("pem_krylov_create_amg", ctx, A, opts, nullptr, M, true, out);
}

extern "C" pem_status pem_krylov_solve(pem_ctx *ctx, pem_krylov *K, const double *db, double *dx, const double *d_minv, double *d_history,
                                       pem_krylov_result *res)
{
    return krylov_solve(ctx, K, db, dx, d_minv, d_history, res, 8, "pem_krylov_solve");
}

extern "C" pem_status pem_krylov_solve_f32(pem_ctx *ctx, pem_krylov *K, const float *db, float *dx, const float *d_minv, double *d_history,
                                           pem_krylov_result *res)
{
    return krylov_solve(ctx, K, db, dx, d_minv, d_history, res, 4, "pem_krylov_solve_f32");
}

extern "C" pem_status pem_krylov_destroy(pem_ctx *ctx, pem_krylov *K)
{
    (void)ctx;
    delete K;   // a context is single-caller and its work is ordered on its stream: the arena may hand the block out again at once
    return PEM_OK;
}

extern "C" pem_status pem_test_krylov_dot(pem_ctx *ctx, int64_t n, int value_bytes, const void *du, const void *dv, double *host_out)
{
    const char *fn = "pem_test_krylov_dot";
    if (!ctx || !host_out || n < 0 || (value_bytes != 4 && value_bytes != 8) || (n > 0 && (!du || !dv))) {
        set_error("%s: null argument, n < 0, or value_bytes not 4 or 8", fn);
        return PEM_E_INVALID;
    }
    PEM_ENTER(ctx);
    DevBuf part;
    PEM_TRY(part.reserve(sizeof(double) * (KR_MAXG + 1)));
    const int G = kr_grid(n);
    double *partial = part.as<double>(), *total = partial + KR_MAXG;
    if (value_bytes == 4)
        PEM_LAUNCH_NAMED(ctx, "krylov_dot", (kr_dot_kernel<float>), G, KR_THREADS, (long long)n, (const KState *)nullptr, (const float *)du,
                         (const float *)dv, partial);
    else
        PEM_LAUNCH_NAMED(ctx, "krylov_dot", (kr_dot_kernel<double>), G, KR_THREADS, (long long)n, (const KState *)nullptr, (const double *)du,
                         (const double *)dv, partial);
    PEM_LAUNCH_NAMED(ctx, "krylov_total", kr_total_kernel, 1, KR_THREADS, (const double *)partial, G, total);
    int64_t bits = 0;
    PEM_TRY(read_scalars(ctx, reinterpret_cast<const int64_t *>(total), 1, &bits));
    PEM_TRY(launch_status(ctx));
    memcpy(host_out, &bits, sizeof(double));
    return PEM_OK;
}
