// amos_block.h -- work-group primitives of the scene-flow kernels (amos_fmat.hip, amos_pnp.hip, amos_dyna.hip, amos_flow.hip): an
// order-preserving compaction and integer sums, by ballot / shuffle and per-wave counts in LDS (no atomics: deterministic, nothing to
// zero).  kThreads is the work-group size (a multiple of 64); every thread of the group calls, sWave holds kThreads / 64 ints.
#pragma once
#include "amos_common.h"

namespace amos {

__device__ __forceinline__ int wave_sum(int v)
{
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

template <int kThreads>
__device__ __forceinline__ int block_sum(int v, int *sWave)
{
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    v = wave_sum(v);
    if (lane == 0) sWave[wv] = v;
    __syncthreads();
    int s = 0;
    for (int w = 0; w < kThreads / 64; w++) s += sWave[w];
    __syncthreads();
    return s;
}

// calls f(i, c) for i < cnt with c the compact index among the i with sel_of(i) (in order), or -1; returns the count
template <int kThreads, typename Sel, typename Fn>
__device__ __forceinline__ int block_compact(int cnt, int *sWave, Sel sel_of, Fn f)
{
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    int total = 0;
    for (int base = 0; base < cnt; base += kThreads) {
        const int i = base + t;
        const bool sel = i < cnt && sel_of(i);
        const unsigned long long b = __ballot(sel);
        if (lane == 0) sWave[wv] = (int)__popcll(b);
        __syncthreads();
        int before = total, all = total;
        for (int w = 0; w < kThreads / 64; w++) {
            if (w < wv) before += sWave[w];
            all += sWave[w];
        }
        if (i < cnt) f(i, sel ? before + (int)__popcll(b & ((1ull << lane) - 1ull)) : -1);
        __syncthreads();
        total = all;
    }
    return total;
}

// Ascending bitonic sort of the n (a power of two) 64-bit keys in LDS by the whole work-group; every thread calls.  The keys on either
// side of a call are separated from the caller's own accesses by the barriers at its start and end.
template <int kThreads>
__device__ __forceinline__ void block_sort_u64(unsigned long long *keys, int n)
{
    __syncthreads();
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (n >> 1); t += kThreads) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;  // the t-th pair of distance j
                const unsigned long long a = keys[lo], b = keys[hi];
                const bool up = (lo & k) == 0;
                if ((a > b) == up) { keys[lo] = b; keys[hi] = a; }
            }
            __syncthreads();
        }
    }
}

}  // namespace amos
