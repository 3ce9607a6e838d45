// kmer_index.hpp — the sorted k-mer table that assess_place.hip and kmer_qv.hip both build and stream a sequence past: 2-bit
// codes and rolling keys, the bitonic sort of (key, tag) entries with its launch schedule, the directory over a key's top 12
// bits, the walk of a byte range tile by tile, and the capped counter. Each file keeps its own table layout, guards, kernels
// and LDS declarations; the kernels here are device function templates that those call.
#pragma once
#include <algorithm>

#include "assess_scan.hpp"

constexpr int KI_DIR_BITS = 12, KI_DIR = 1 << KI_DIR_BITS;   // the directory: KI_DIR + 1 offsets into the sorted keys

__device__ inline uint32_t code_of(uint8_t c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4; }

inline unsigned blocks_for(int64_t items, int64_t per_block, int64_t most) {
    return (unsigned)std::max<int64_t>(1, std::min(most, (items + per_block - 1) / per_block));
}

// the rolling pair of keys of the last k codes, k <= 32: forward, first byte highest; reverse complement, last byte's
// complement highest. A caller that reads only one of them, with k known to the compiler, pays for that one alone.
struct Roll {
    uint64_t fwd = 0, rev = 0, mask; int top, run = 0, k;
    __device__ explicit Roll(int k_) : mask(~0ull >> (64 - 2 * k_)), top(2 * (k_ - 1)), k(k_) {}
    __device__ inline void push(uint32_t c) {
        fwd = ((fwd << 2) | (c & 3)) & mask;
        rev = (rev >> 2) | ((uint64_t)(3 - (c & 3)) << top);
        run = c < 4 ? run + 1 : 0;
    }
    __device__ inline bool keyed() const { return run >= k; }
    __device__ inline uint64_t canon() const { return fwd < rev ? fwd : rev; }
};

// ---- the sort ---------------------------------------------------------------------------------------------------------------
// A bitonic network in which every comparison is ascending (the first step of a merge mirrors its partner), so that a table of
// any size sorts in place as if padded with infinite entries: spans of SPAN entries in LDS, the wider steps one launch each.
// The order of two entries is a policy: by_tag says whether less() looks at the tags at all.
struct ByKey {   // by key alone: a tag is loaded only to be swapped
    static constexpr bool by_tag = false;
    __device__ static bool less(uint64_t ka, uint32_t, uint64_t kb, uint32_t) { return ka < kb; }
};
struct TriedThenKey {   // a tag's top bit marks an untried entry: those sort behind all others, then by key
    static constexpr bool by_tag = true;
    __device__ static bool less(uint64_t ka, uint32_t ta, uint64_t kb, uint32_t tb) {
        const uint32_t ua = ta >> 31, ub = tb >> 31;
        return ua != ub ? ua < ub : ka < kb;
    }
};
template <typename Order, typename I>
__device__ inline void order_pair(uint64_t* keys, uint32_t* tags, I i, I l) {
    const uint64_t ki = keys[i], kl = keys[l];
    uint32_t ti = 0, tl = 0;
    if (Order::by_tag) { ti = tags[i]; tl = tags[l]; }
    if (!Order::less(kl, tl, ki, ti)) return;
    if (!Order::by_tag) { ti = tags[i]; tl = tags[l]; }
    keys[i] = kl; tags[i] = tl; keys[l] = ki; tags[l] = ti;
}

// pair q of a step of width j: the lower index has bit j clear; its partner is mirrored in the block of 2 j (the first step of a
// merge) or j higher (every other step)
__device__ inline int64_t pair_low(int64_t q, int64_t j) { return ((q & ~(j - 1)) << 1) | (q & (j - 1)); }
__device__ inline int64_t pair_high(int64_t i, int64_t j, bool mirror) { return mirror ? i ^ (2 * j - 1) : i | j; }

// tail == 0: the merges of 2 .. SPAN entries, each in full; tail == 1: the steps of width SPAN / 2 .. 1 of a wider merge
template <int SPAN, typename Order>
__device__ inline void sort_spans(uint64_t* keys, uint32_t* tags, int64_t n, int tail) {
    __shared__ uint64_t s_key[SPAN];
    __shared__ uint32_t s_tag[SPAN];
    for (int64_t base = (int64_t)blockIdx.x * SPAN; base < n; base += (int64_t)gridDim.x * SPAN) {
        __syncthreads();
        for (int i = threadIdx.x; i < SPAN; i += AS_THREADS) {
            const bool in = base + i < n;   // behind the table: infinite entries, which never move
            s_key[i] = in ? keys[base + i] : ~0ull;
            s_tag[i] = in ? tags[base + i] : ~0u;
        }
        __syncthreads();
        for (int k = tail ? SPAN : 2; k <= SPAN; k <<= 1) {
            for (int j = k >> 1; j >= 1; j >>= 1) {
                const bool mirror = !tail && j == (k >> 1);
                for (int q = threadIdx.x; q < SPAN / 2; q += AS_THREADS) {
                    const int i = (int)pair_low(q, j);
                    order_pair<Order>(s_key, s_tag, i, (int)pair_high(i, j, mirror));
                }
                __syncthreads();
            }
        }
        for (int i = threadIdx.x; i < SPAN; i += AS_THREADS)
            if (base + i < n) { keys[base + i] = s_key[i]; tags[base + i] = s_tag[i]; }
    }
}

// one step of width j >= SPAN: a lane per pair, in global memory
template <typename Order>
__device__ inline void sort_global_step(uint64_t* keys, uint32_t* tags, int64_t n, int64_t j, bool mirror) {
    for (int64_t q = (int64_t)blockIdx.x * AS_THREADS + threadIdx.x;; q += (int64_t)gridDim.x * AS_THREADS) {
        const int64_t i = pair_low(q, j), l = pair_high(i, j, mirror);
        if (i >= n) break;   // (i grows with q)
        if (l >= n) continue;
        order_pair<Order>(keys, tags, i, l);
    }
}

// the launches that sort up to `entries` entries: local(tail) launches the span kernel, global(j, mirror) one wide step. With
// P = entries rounded up to a power of two and m = max(0, log2(P / span)), that is 1 + m + m (m + 1) / 2 launches.
template <typename Local, typename Global>
inline void sort_schedule(int64_t entries, int64_t span, Local local, Global global) {
    local(0);
    for (int64_t w = 2 * span; (w >> 1) < entries; w <<= 1) {
        for (int64_t j = w >> 1; j >= span; j >>= 1) global(j, j == (w >> 1));
        local(1);
    }
}

// ---- the directory ----------------------------------------------------------------------------------------------------------
// the first e in [lo, hi) with keys[e] >= key, or hi
__device__ inline int64_t first_at_least(const uint64_t* keys, int64_t lo, int64_t hi, uint64_t key) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// Bucket b holds the keys in [b << shift, (b + 1) << shift): the directory's entry b is where they begin among the n sorted keys.
__device__ inline uint32_t dir_entry(const uint64_t* keys, int64_t n, int b, int shift) {
    return (uint32_t)first_at_least(keys, 0, n, (uint64_t)b << shift);
}
// the first entry of key's bucket (the directory: KI_DIR + 1 offsets, best in LDS) with a key >= key, and the bucket's end
struct DirHit { int64_t e, top; };
__device__ inline DirHit dir_find(const uint32_t* s_dir, const uint64_t* keys, uint64_t key, int shift) {
    const uint32_t b = (uint32_t)(key >> shift);
    const int64_t top = s_dir[b + 1];
    return {first_at_least(keys, s_dir[b], top, key), top};
}

// ---- the walk ---------------------------------------------------------------------------------------------------------------
// The bytes [lo, hi) of `bases`, which the n ranges of `off` divide, pass the grid's workgroups in tiles of TILE. A tile and
// its (k - 1)-byte halo go to s_code (TILE + k - 1 bytes of LDS) as codes; per_tile() runs behind that barrier; a lane then
// rolls the keys of TILE / AS_THREADS consecutive offsets from the range that owns its first one, and visit(roll, pos, t,
// start) is called for every offset pos whose k bytes are all bases of one range t, which begins at `start`. Nothing outside
// [lo, hi) is read and t stays below n whatever the offsets hold.
template <int TILE, typename PerTile, typename Visit>
__device__ inline void tile_walk(const uint8_t* bases, const int64_t* off, int64_t n, int64_t lo, int64_t hi, int k,
                                 uint8_t* s_code, PerTile per_tile, Visit visit) {
    constexpr int PER = TILE / AS_THREADS;
    for (int64_t g0 = lo + (int64_t)blockIdx.x * TILE; g0 < hi; g0 += (int64_t)gridDim.x * TILE) {
        __syncthreads();   // the previous tile has been read
        for (int i = threadIdx.x; i < TILE + k - 1; i += AS_THREADS) s_code[i] = g0 + i < hi ? code_of(bases[g0 + i]) : 4;
        __syncthreads();
        per_tile();
        const int i0 = threadIdx.x * PER;
        if (g0 + i0 >= hi) continue;
        int64_t t = owner_of(off, n, g0 + i0);
        int64_t start = off[t], end = off[t + 1];
        Roll r(k);
        for (int q = 0; q < k - 1; q++) r.push(s_code[i0 + q]);
        for (int m = 0; m < PER; m++) {
            r.push(s_code[i0 + k - 1 + m]);
            const int64_t pos = g0 + i0 + m;
            if (pos >= hi) break;
            while (pos >= end && t + 1 < n) { t++; start = end; end = off[t + 1]; }
            if (!r.keyed() || pos + k > end) continue;
            visit(r, pos, t, start);
        }
    }
}

// one more on a counter that stays at its cap, so it cannot wrap: the overshoot is bounded by the lanes in flight
__device__ inline void add_capped(uint32_t* counter, uint32_t cap) {
    if (__hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < cap) atomicAdd(counter, 1u);
}
