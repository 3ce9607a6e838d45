// assess_scan.hpp — the small device helpers that assess.hip, assess_place.hip and kmer_qv.hip share: the 256-byte rounding of
// their layouts, the owner of an index among ranges, a wave sum, a block reduction, a one-block exclusive scan and the flush of
// a histogram kept in LDS.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

constexpr int AS_THREADS = 256;

__host__ __device__ inline int64_t up256(int64_t x) { return (x + 255) & ~(int64_t)255; }

// the last p in [0, n) with off[p] <= s, for off[0] <= s < off[n]: empty ranges are passed over
__device__ inline int64_t owner_of(const int64_t* off, int64_t n, int64_t s) {
    int64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (off[mid] <= s) lo = mid; else hi = mid - 1;
    }
    return lo;
}

template <typename T>
__device__ inline T wave_sum(T v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// all threads of the block get op over every thread's v (a 64-bit integer); lds: T [AS_THREADS / 64]
template <typename T, typename F>
__device__ inline T block_reduce(T v, T* lds, F op) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = op(v, (T)__shfl_xor((unsigned long long)v, d, 64));
    __syncthreads();   // lds is free again
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    v = lds[0];
    for (int i = 1; i < AS_THREADS / 64; i++) v = op(v, lds[i]);
    return v;
}
struct as_add {
    template <typename T>
    __device__ T operator()(T a, T b) const { return a + b; }
};

// the non-zero cells of a block's histogram in LDS, added to out[0..n) by 64-bit atomics
__device__ inline void lds_hist_flush(const uint32_t* s_hist, int n, int64_t* out) {
    for (int i = threadIdx.x; i < n; i += AS_THREADS)
        if (s_hist[i]) atomicAdd((unsigned long long*)&out[i], (unsigned long long)s_hist[i]);
}

// one block of AS_THREADS: exclusive scan of f(p) over p < n into out[0..n] (out[n] = the sum); returns the sum to every thread.
// lds: int64 [AS_THREADS / 64]
template <typename F>
__device__ inline int64_t block_scan_to(int64_t n, int64_t* out, int64_t* lds, F f) {
    const int64_t per = (n + AS_THREADS - 1) / AS_THREADS;
    const int64_t k0 = min(n, (int64_t)threadIdx.x * per), k1 = min(n, k0 + per);
    int64_t s = 0;
    for (int64_t k = k0; k < k1; k++) s += f(k);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int64_t x = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) lds[w] = x;
    __syncthreads();
    int64_t off = 0, sum = 0;
    for (int i = 0; i < AS_THREADS / 64; i++) { off += i < w ? lds[i] : 0; sum += lds[i]; }
    __syncthreads();
    off += x - s;
    for (int64_t k = k0; k < k1; k++) { out[k] = off; off += f(k); }
    if (threadIdx.x == 0) out[n] = sum;
    return sum;
}
