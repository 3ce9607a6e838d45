// assess_scan.hpp — the small device helpers that assess.hip and assess_place.hip share: the 256-byte rounding of their scratch
// layouts, a wave sum and a one-block exclusive scan.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

constexpr int AS_THREADS = 256;

__host__ __device__ inline int64_t up256(int64_t x) { return (x + 255) & ~(int64_t)255; }

template <typename T>
__device__ inline T wave_sum(T v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
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
