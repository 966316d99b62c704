// scan_chain.h -- the device side of the single-launch chained scan, shared by its two users: scan_mid_kernel (primitives.hip)
// and the row classification of step 1, which scans its own row totals (step1.hip).  Up to SCAN_MID_BLOCKS blocks; a block
// takes its place in the order by TICKET, publishes its total in an 8-byte valid-tagged word and sums the words of every
// earlier ticket (at most 127: two per lane of one wave, one round trip).  See scan_mid_kernel for why this cannot deadlock.
// One set of words = SCAN_MID_BLOCKS totals + one word holding two ints: blocks done, next ticket; all zero between scans.
#pragma once
#include "pem_internal.h"

namespace pem {

constexpr int SCAN_MID_BLOCKS = 128;
constexpr int SCAN_MID_SETS = 3;   // scan_mid_kernel's two arrays, and the row classification's own
constexpr unsigned long long SCAN_MID_VALID = 1ull << 63;
constexpr size_t SCAN_MID_SET_WORDS = SCAN_MID_BLOCKS + 2;

template <typename T> __device__ __forceinline__ T wave_inclusive_scan(T v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        T t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

template <typename T> __device__ __forceinline__ T wave_reduce_sum(T v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ int *scan_chain_ctl(unsigned long long *state) { return reinterpret_cast<int *>(state + SCAN_MID_BLOCKS); }   // done, ticket

// one thread of the block: its place in the order
__device__ __forceinline__ int scan_chain_ticket(unsigned long long *state) { return atomicAdd(&scan_chain_ctl(state)[1], 1); }

// lane 0 of one wave: the block's total, for the later tickets (62 bits: a block's own sum can exceed 2^31 when the scan as a
// whole overflows -- the caller flags that)
__device__ __forceinline__ void scan_chain_publish(unsigned long long *state, const int blk, const long long btotal)
{
    __hip_atomic_store(&state[blk], SCAN_MID_VALID | (unsigned long long)btotal, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one whole wave, after the publish: the sum of the totals of tickets < blk.  The wait is bounded; should it ever run out (it
// cannot), FLAG_INTERNAL makes the host fail the call instead of returning a wrong scan.
__device__ __forceinline__ long long scan_chain_lookback(unsigned long long *state, const int blk, const int lane, int *__restrict__ flags)
{
    long long excl = 0;
    bool ok = false;
    for (long long polls = 0; polls < (1ll << 24) && !ok; ++polls) {
        const unsigned long long a = lane < blk ? __hip_atomic_load(&state[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : SCAN_MID_VALID;
        const unsigned long long b = 64 + lane < blk ? __hip_atomic_load(&state[64 + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : SCAN_MID_VALID;
        if (__ballot(!(a & SCAN_MID_VALID) || !(b & SCAN_MID_VALID)) == 0) {
            excl = wave_reduce_sum((long long)(a & ~SCAN_MID_VALID) + (long long)(b & ~SCAN_MID_VALID));
            ok = true;
        } else {
            __builtin_amdgcn_s_sleep(1);
        }
    }
    if (!ok && lane == 0) flags[FLAG_INTERNAL] = 1;
    return excl;
}

// one thread of the block, once the block has read what it needed: the last block to get here has seen every other block do so
// and clears the words for the next scan
__device__ __forceinline__ void scan_chain_done(unsigned long long *state, const int nblk)
{
    int *ctl = scan_chain_ctl(state);
    if (atomicAdd(&ctl[0], 1) == nblk - 1) {
        for (int b = 0; b < nblk; ++b) __hip_atomic_store(&state[b], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&ctl[0], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&ctl[1], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the context's look-back words (SCAN_MID_SETS sets, allocated and zeroed on first use)
pem_status scan_mid_state(pem_ctx *ctx);

}  // namespace pem
