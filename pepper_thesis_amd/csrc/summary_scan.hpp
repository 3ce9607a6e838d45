// summary_scan.hpp — the exclusive scans of the summary pipelines (K3) as device templates; the scan kernels themselves
// live in summary_front.hip (tiles, k_scan_i32) and summary_builder.hip (per-site arrays).
#pragma once
#include "summary_types.hpp"

namespace pvsum {

// ---- K3 -------------------------------------------------------------------------------------------
// Exclusive scans of the pipeline's small arrays (tiles, 1024-column blocks, sites). A thread owns SCAN_V consecutive
// values per pass, a 1024-thread workgroup 8192. These kernels are chains of dependent memory round trips, not work,
// so the chains are kept short:
//  * arrays whose length the host knows (tiles, blocks) run as one workgroup looping over passes, every thread
//    summing the 16 wave totals itself (no carry cell, two barriers per pass);
//  * the per-site arrays (length = diag[D_NSITES], 17.9 k in the benchmark's 16-region batches: three passes) run one
//    workgroup per 8192-entry chunk. A chunk's carry is the sum of everything before it, which the workgroup adds up
//    itself from the input (independent coalesced loads: at most n^2 / 16 k loads in all, nothing at these sizes)
//    instead of waiting for its neighbours; the chunk's own values are loaded together WITH the length (the arrays
//    are max_sites long, the grid covers max_sites) and masked once it has arrived. The workgroup holding the last
//    entry publishes the totals. k_scan_outputs runs its two scans side by side.
// What used to be separate one-thread kernels behind a scan (limit checks, publishing the result counters) runs in the
// scan's first thread.
constexpr int SCAN_V = 8;
constexpr int64_t SCAN_PASS = 1024 * SCAN_V;
constexpr int SCAN_SPEC_CHUNKS = 3;  // chunks below this add up their carry before the length has arrived
// Loads go through a sized raw buffer: entries past `elems` read as zero without a branch per load, so all of a
// thread's loads are in flight together. (Byte offsets are 32-bit: arrays here stay below 2^31 bytes, n_cols < 2^31.)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t scan_rsrc(const void* p, int64_t elems, int esz) {
    const int64_t bytes = elems > 0 ? elems * esz : 0;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)(bytes > 0x7fffffff ? 0x7fffffff : bytes),
                                             0x00020000);
}
__device__ __forceinline__ unsigned scan_voff(int64_t i, int esz) {
    const int64_t b = i * esz;
    return b > 0x7fffffff ? 0x80000000u : (unsigned)b;
}
__device__ __forceinline__ int32_t scan_ld(__amdgpu_buffer_rsrc_t r, int64_t i, int32_t) {
    return (int32_t)__builtin_amdgcn_raw_buffer_load_b32(r, scan_voff(i, 4), 0, 0);
}
__device__ __forceinline__ int64_t scan_ld(__amdgpu_buffer_rsrc_t r, int64_t i, int64_t) {
    typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
    const u32x2_t w = __builtin_amdgcn_raw_buffer_load_b64(r, scan_voff(i, 8), 0, 0);
    const unsigned lo = w[0], hi = w[1];
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
typedef unsigned scan_u32x4 __attribute__((ext_vector_type(4)));
// sum of the 16 bytes at entry i (4 int32 or 2 int64 values)
__device__ __forceinline__ int64_t scan_ld16_sum(__amdgpu_buffer_rsrc_t r, int64_t i, int32_t) {
    const scan_u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(r, scan_voff(i, 4), 0, 0);
    const unsigned w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
    return (int64_t)(int32_t)w0 + (int32_t)w1 + (int64_t)(int32_t)w2 + (int32_t)w3;
}
__device__ __forceinline__ int64_t scan_ld16_sum(__amdgpu_buffer_rsrc_t r, int64_t i, int64_t) {
    const scan_u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(r, scan_voff(i, 8), 0, 0);
    const unsigned w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
    return (int64_t)(((uint64_t)w1 << 32) | w0) + (int64_t)(((uint64_t)w3 << 32) | w2);
}
// A thread's SCAN_V consecutive values. The vector memory pipe of the one CU a scan workgroup sits on is what these
// kernels wait for (about 18 cycles per load instruction, 16 waves), so the values come as 16-byte loads; only a thread
// whose run crosses `lim` loads entry by entry.
__device__ __forceinline__ void scan_load(const int32_t* in, int64_t i0, int64_t lim, int32_t (&v)[SCAN_V]) {
    const __amdgpu_buffer_rsrc_t r = scan_rsrc(in, lim, 4);
    if (i0 + SCAN_V <= lim || i0 >= lim) {
#pragma unroll
        for (int q = 0; q < SCAN_V / 4; q++) {
            const scan_u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(r, scan_voff(i0 + 4 * q, 4), 0, 0);
            const unsigned w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
            v[4 * q] = (int32_t)w0; v[4 * q + 1] = (int32_t)w1; v[4 * q + 2] = (int32_t)w2; v[4 * q + 3] = (int32_t)w3;
        }
    } else {
#pragma unroll
        for (int e = 0; e < SCAN_V; e++) v[e] = scan_ld(r, i0 + e, int32_t());
    }
}
// (8-byte values: one load each, whole or not at all, so no branch - a branch here makes the compiler wait for the
// loads at its end, ahead of the loads that should follow them out)
__device__ __forceinline__ void scan_load(const int64_t* in, int64_t i0, int64_t lim, int64_t (&v)[SCAN_V]) {
    const __amdgpu_buffer_rsrc_t r = scan_rsrc(in, lim, 8);
#pragma unroll
    for (int e = 0; e < SCAN_V; e++) v[e] = scan_ld(r, i0 + e, int64_t());
}
template <typename T>
__device__ __forceinline__ void scan_mask(int64_t i0, int64_t n, T (&v)[SCAN_V]) {
#pragma unroll
    for (int e = 0; e < SCAN_V; e++) v[e] = i0 + e < n ? v[e] : (T)0;
}
// this thread's share of sum(in[0 .. c0)), c0 a multiple of SCAN_PASS and at most `lim`: 16 bytes per load, lanes side
// by side
template <typename T>
__device__ __forceinline__ int64_t scan_carry_part(const T* in, int64_t c0, int64_t lim) {
    constexpr int PER = 16 / (int)sizeof(T);  // values per load
    const __amdgpu_buffer_rsrc_t r = scan_rsrc(in, lim, (int)sizeof(T));
    int64_t pre = 0;
    for (int64_t j0 = (int64_t)threadIdx.x * PER; j0 < c0; j0 += SCAN_PASS) {
        int64_t q[SCAN_V / PER];
#pragma unroll
        for (int e = 0; e < SCAN_V / PER; e++) q[e] = scan_ld16_sum(r, j0 + 1024 * PER * e, T());
#pragma unroll
        for (int e = 0; e < SCAN_V / PER; e++) pre += q[e];
    }
    return pre;
}
// the same for the first SCAN_SPEC_CHUNKS chunks: a fixed number of loads (those at or past c0 read as zero: c0 is a
// multiple of every load's span), all in flight at once
template <typename T>
__device__ __forceinline__ int64_t scan_carry_part_spec(const T* in, int64_t c0) {
    constexpr int PER = 16 / (int)sizeof(T);
    constexpr int NL = SCAN_V * (SCAN_SPEC_CHUNKS - 1) / PER;
    const __amdgpu_buffer_rsrc_t r = scan_rsrc(in, c0, (int)sizeof(T));
    int64_t q[NL];
#pragma unroll
    for (int k = 0; k < NL; k++) q[k] = scan_ld16_sum(r, ((int64_t)threadIdx.x + 1024 * k) * PER, T());
    int64_t pre = 0;
#pragma unroll
    for (int k = 0; k < NL; k++) pre += q[k];
    return pre;
}
// the scans' length: a vector load (kept in program order with the value loads around it: issued before the carry
// loads, waited for after them), then made uniform
__device__ __forceinline__ int64_t scan_len_issue(const int64_t* p) { return scan_ld(scan_rsrc(p, 1, 8), 0, int64_t()); }
__device__ __forceinline__ int64_t scan_len_uniform(int64_t v) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
// one pass over v[] (zero beyond n): out[i0..] = carry + exclusive prefix; returns carry + the pass total.
// carry = `carry` (same in every thread) + the sum of `part` over the workgroup. s_w: 32 cells, reusable after the
// closing barrier, which only a caller with another pass to run asks for (it also waits for the stores).
template <typename T>
__device__ __forceinline__ int64_t scan_pass(const T (&v)[SCAN_V], T* out, int64_t i0, int64_t n, int64_t carry,
                                             int64_t part, int64_t* s_w, bool again = false) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int64_t sum = 0;
#pragma unroll
    for (int e = 0; e < SCAN_V; e++) sum += (int64_t)v[e];
    const int64_t inc = wave_incl_scan(sum, lane);
    const int64_t pinc = wave_incl_scan(part, lane);
    if (lane == 63) { s_w[wv] = inc; s_w[16 + wv] = pinc; }
    __syncthreads();
    int64_t woff = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const int64_t w = s_w[k];
        woff += k < wv ? w : 0;
        tot += w;
        carry += s_w[16 + k];
    }
    int64_t run = carry + woff + inc - sum;
    T o[SCAN_V];
#pragma unroll
    for (int e = 0; e < SCAN_V; e++) { o[e] = (T)run; run += (int64_t)v[e]; }
    if (i0 + SCAN_V <= n) {  // 16-byte stores (i0 is a multiple of SCAN_V, the arrays are 256-byte aligned)
        typedef T ovec __attribute__((ext_vector_type(16 / sizeof(T))));
        constexpr int PER = 16 / (int)sizeof(T);
#pragma unroll
        for (int q = 0; q < SCAN_V / PER; q++) {
            ovec w;
#pragma unroll
            for (int e = 0; e < PER; e++) w[e] = o[PER * q + e];
            *reinterpret_cast<ovec*>(out + i0 + PER * q) = w;
        }
    } else {
#pragma unroll
        for (int e = 0; e < SCAN_V; e++) if (i0 + e < n) out[i0 + e] = o[e];
    }
    if (again) __syncthreads();
    return carry + tot;
}
// one workgroup, n known to the host
template <typename T>
__device__ __forceinline__ int64_t block_excl_scan(const T* in, T* out, int64_t n, int64_t* s_w) {
    int64_t carry = 0;
    for (int64_t b = 0; b == 0 || b < n; b += SCAN_PASS) {
        const int64_t i0 = b + (int64_t)threadIdx.x * SCAN_V;
        T v[SCAN_V];
        scan_load(in, i0, n, v);
        carry = scan_pass(v, out, i0, n, carry, 0, s_w, b + SCAN_PASS < n);
    }
    return carry;
}
// grid of the per-site scans
static inline unsigned scan_chunks(int64_t cap) { return (unsigned)std::max<int64_t>(1, (cap + SCAN_PASS - 1) / SCAN_PASS); }

}  // namespace pvsum
