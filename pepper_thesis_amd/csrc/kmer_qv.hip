// kmer_qv.hip — score an assembly by the support its k-mers have in the reads: a k-mer of the assembly that too few reads
// contain is taken to be an error (`pepper kmer_qv`).
//
// The rule is in include/pepper_hip.h (pv_kmer_support). The reads are the large side and come batch by batch, so the table
// is made of the assembly's k-mers: its size is known before the first read arrives. One entry per assembly position, sorted
// by canonical key on the device; the reads stream past it and add to one counter per distinct key. All on one stream, no host
// read-back:
//   pv_kmer_table_build_dev
//     k_km_setup        one block: the offsets' check, the summed length, what the table needs, the header, the status
//     k_km_keys         one lane per stretch of KM_STRETCH positions: rolling forward and reverse keys -> (canonical key,
//                       position); a position without a key gets KM_NONE, which sorts behind every key; counters 0
//     k_km_sort_local   the bitonic network of assess_place.hip (every comparison ascending, the first step of a merge
//     k_km_sort_global  mirrored, so a table of any size sorts as if padded with infinite entries), ordered by key alone
//     k_km_dir          where the keys of each value of their own top 12 bits (of 2 k) begin, and the number of keyed entries
//   pv_kmer_count_reads_dev
//     k_km_count        THE HOT PATH. A workgroup takes PV_KMER_TILE read bytes and a (k - 1)-byte halo into LDS as codes
//                       (0..3, 4 = no base); a lane rolls the keys of 16 consecutive offsets, skips what does not lie in one
//                       read, finds the canonical key (directory in LDS, then a binary search in L2) and adds one to the
//                       counter of the first entry with that key, unless it has reached the cap
//   pv_kmer_support_dev
//     k_km_sup_setup    one block: the table and the offsets checked against each other, the segment offsets, zeroed sums
//     k_km_gather       one lane per sorted entry: the count of its key (the first equal entry's, capped) to its position
//     k_km_sums         a workgroup per segment: unsupported positions of the segment, the contig's sums, the histogram in LDS
//     k_km_run_count    a workgroup per KM_RUN_TILE positions: how many runs start and how many end there
//     k_km_run_scan     one block: the tiles' offsets, the number of runs, PV_ERR_CAPACITY, the contigs' positions without a key
//     k_km_run_write    the j-th start and the j-th end of the flat order are one run: (contig, first) and (last) written apart
//     k_km_poison       under a status other than PV_OK and PV_ERR_CAPACITY: -1 in every output
// --completeness (the second section of the header): the read k-mers the assembly lacks, in an open-addressing table of their own
//   pv_kmer_reads_table_init_dev
//     k_kr_init         every slot empty, the head
//   pv_kmer_count_reads_all_dev
//     k_km_count_all    k_km_count with a part filter and a miss path: a key the assembly lacks claims or finds its slot (linear
//                       probing from mix(key), one 64-bit compare-and-swap on an empty slot) and adds one there under the cap
//   pv_kmer_reads_flush_dev
//     k_kr_flush_setup  one lane: the head checked, {0, status, dropped, slots}, status and dropped reset
//     k_kr_flush        a lane per slot: the histogram of the counts in LDS, the table emptied
//   pv_kmer_spectrum_dev
//     k_km_spec_setup   one lane: the table's status
//     k_km_spectrum     a lane per sorted entry: the first of equal keys adds its (multiplicity, count) to the spectrum in LDS
// The counters are integer atomics: the result does not depend on tile size, workgroup count or the order of the calls.
#include <algorithm>

#include "assess_scan.hpp"
#include "pv_common.hpp"

namespace {

constexpr int KM_TILE = PV_KMER_TILE;
constexpr int KM_PER = KM_TILE / AS_THREADS;    // consecutive offsets of a lane of the count
constexpr int KM_HALO = PV_KMER_MAX_K - 1;
constexpr int KM_STRETCH = 32;                  // consecutive positions of a lane of the key kernel
constexpr int KM_SORT = PV_KMER_SORT_SPAN;      // entries a workgroup sorts in LDS
constexpr int KM_DIR_BITS = 12, KM_DIR = 1 << KM_DIR_BITS;
constexpr int KM_RUN_PER = 8, KM_RUN_TILE = AS_THREADS * KM_RUN_PER;
constexpr uint64_t KM_NONE = ~0ull;             // no key has more than 62 bits
constexpr uint32_t KM_NO_KEY = PV_KMER_NO_KEY;
constexpr int64_t KM_MAGIC = 0x5651524D4B5650ll;
constexpr int KM_HEAD = 256;
static_assert(KM_TILE % AS_THREADS == 0 && KM_SORT % AS_THREADS == 0, "tile and span");

// the table: offsets in bytes, all multiples of 256. N = the summed assembly length, T = ceil(N / KM_RUN_TILE).
//   head    int64 [32]          {magic, k, cap, n_asm, N, status, keyed entries}
//   dir     uint32 [KM_DIR + 1] the sorted keys' directory
//   keys    uint64 [N]          sorted; KM_NONE for a position without a key
//   tags    uint32 [N]          the flat position a sorted key belongs to
//   cnt     uint32 [N]          by sorted entry: the occurrences of its key in the reads, kept on the first of equal keys
//   posc    uint32 [N]          by flat position: its count as the last summary gathered it
//   tile_cs, tile_ce int64 [T]      runs that start / end in a tile
//   tile_s, tile_e   int64 [T + 1]  their exclusive offsets
struct Layout { int64_t dir, keys, tags, cnt, posc, tile_cs, tile_ce, tile_s, tile_e, total; };
__host__ __device__ inline int64_t run_tiles(int64_t N) { return (N + KM_RUN_TILE - 1) / KM_RUN_TILE; }
__host__ __device__ inline Layout km_layout(int64_t N) {
    Layout y;
    const int64_t T = run_tiles(N);
    y.dir = KM_HEAD;
    y.keys = y.dir + up256((KM_DIR + 1) * 4);
    y.tags = y.keys + up256(N * 8);
    y.cnt = y.tags + up256(N * 4);
    y.posc = y.cnt + up256(N * 4);
    y.tile_cs = y.posc + up256(N * 4);
    y.tile_ce = y.tile_cs + up256(T * 8);
    y.tile_s = y.tile_ce + up256(T * 8);
    y.tile_e = y.tile_s + up256((T + 1) * 8);
    y.total = y.tile_e + up256((T + 1) * 8);
    return y;
}
// a bound of the positions a table of `bytes` can hold: it sizes grids and the sort's depth, the kernels take N from the head
inline int64_t positions_bound(int64_t bytes) { return std::max<int64_t>(1, (bytes - km_layout(0).total) / 20 + 1); }

enum { H_MAGIC, H_K, H_CAP, H_NASM, H_N, H_STATUS, H_KEYED };

struct Table {
    int64_t N; int k; uint32_t cap; int shift;
    uint32_t* dir; uint64_t* keys; uint32_t* tags; uint32_t* cnt; uint32_t* posc;
    int64_t *tile_cs, *tile_ce, *tile_s, *tile_e;
};
__device__ inline int64_t* head_of(void* table) { return (int64_t*)table; }
__device__ inline bool table_ok(const void* table) {
    const int64_t* h = (const int64_t*)table;
    return h[H_MAGIC] == KM_MAGIC && h[H_STATUS] == PV_OK;
}
__device__ inline Table table_of(void* table) {
    const int64_t* h = head_of(table);
    const Layout y = km_layout(h[H_N]);
    uint8_t* b = (uint8_t*)table;
    return {h[H_N], (int)h[H_K], (uint32_t)h[H_CAP], 2 * (int)h[H_K] - KM_DIR_BITS,
            (uint32_t*)(b + y.dir), (uint64_t*)(b + y.keys), (uint32_t*)(b + y.tags), (uint32_t*)(b + y.cnt), (uint32_t*)(b + y.posc),
            (int64_t*)(b + y.tile_cs), (int64_t*)(b + y.tile_ce), (int64_t*)(b + y.tile_s), (int64_t*)(b + y.tile_e)};
}

// the last p in [0, n) with off[p] <= s, for off[0] <= s < off[n]: empty ranges are passed over
__device__ inline int64_t owner_of(const int64_t* off, int64_t n, int64_t s) {
    int64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (off[mid] <= s) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ inline uint32_t code_of(uint8_t c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4; }

// the rolling pair of keys of the last k codes: forward, first byte highest; reverse complement, last byte's complement highest
struct Roll {
    uint64_t fwd = 0, rev = 0, mask; int top, run = 0, k;
    __device__ explicit Roll(int k_) : mask((1ull << (2 * k_)) - 1), top(2 * (k_ - 1)), k(k_) {}
    __device__ inline void push(uint32_t c) {
        fwd = ((fwd << 2) | (c & 3)) & mask;
        rev = (rev >> 2) | ((uint64_t)(3 - (c & 3)) << top);
        run = c < 4 ? run + 1 : 0;
    }
    __device__ inline bool keyed() const { return run >= k; }
    __device__ inline uint64_t canon() const { return fwd < rev ? fwd : rev; }
};

// all threads of the block get the sum of every thread's v; lds: int64 [AS_THREADS / 64]
__device__ inline int64_t block_sum(int64_t v, int64_t* lds) {
    v = wave_sum(v);
    __syncthreads();   // lds is free again
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    v = 0;
    for (int i = 0; i < AS_THREADS / 64; i++) v += lds[i];
    return v;
}

// ---- the table --------------------------------------------------------------------------------------------------------------
struct BuildArgs {
    const uint8_t* A; const int64_t* a_off; int64_t n_asm;
    int k; int64_t cap;
    void* table; int64_t table_bytes;
    int64_t* counts;   // {keyed entries, status, first bad contig or -1, table bytes needed}
};

__global__ __launch_bounds__(AS_THREADS) void k_km_setup(BuildArgs g) {
    __shared__ unsigned long long s_bad;
    if (threadIdx.x == 0) s_bad = KM_NONE;
    __syncthreads();
    for (int64_t p = threadIdx.x; p < g.n_asm; p += AS_THREADS)
        if (g.a_off[p + 1] < g.a_off[p]) atomicMin(&s_bad, (unsigned long long)p);
    __syncthreads();
    if (threadIdx.x != 0) return;
    const unsigned long long bad = s_bad;
    const int64_t N = bad != KM_NONE || g.n_asm == 0 ? 0 : g.a_off[g.n_asm] - g.a_off[0];
    const int64_t need = km_layout(N < (1ll << 31) ? N : (1ll << 31)).total;
    const int64_t status = bad != KM_NONE ? PV_ERR_INVALID : (N >= (1ll << 31) || need > g.table_bytes) ? PV_ERR_LIMIT : PV_OK;
    int64_t* h = head_of(g.table);
    h[H_MAGIC] = KM_MAGIC; h[H_K] = g.k; h[H_CAP] = g.cap; h[H_NASM] = g.n_asm;
    h[H_N] = status == PV_OK ? N : 0; h[H_STATUS] = status; h[H_KEYED] = 0;
    g.counts[0] = 0; g.counts[1] = status; g.counts[2] = bad != KM_NONE ? (int64_t)bad : -1; g.counts[3] = need;
}

__global__ __launch_bounds__(AS_THREADS) void k_km_keys(BuildArgs g) {
    if (!table_ok(g.table)) return;
    const Table tb = table_of(g.table);
    const int64_t base = tb.N ? g.a_off[0] : 0, stretches = (tb.N + KM_STRETCH - 1) / KM_STRETCH;
    for (int64_t s = (int64_t)blockIdx.x * AS_THREADS + threadIdx.x; s < stretches; s += (int64_t)gridDim.x * AS_THREADS) {
        const int64_t f0 = s * KM_STRETCH;
        // the contig of the lane's first position, then forward from it; a k-mer lies inside one contig
        int64_t p = owner_of(g.a_off, g.n_asm, base + f0);
        int64_t end = g.a_off[p + 1] - base;
        Roll r(tb.k);
        for (int q = 0; q < tb.k - 1; q++) r.push(f0 + q < tb.N ? code_of(g.A[base + f0 + q]) : 4);
        for (int m = 0; m < KM_STRETCH; m++) {
            const int64_t f = f0 + m;
            if (f >= tb.N) break;
            r.push(f + tb.k - 1 < tb.N ? code_of(g.A[base + f + tb.k - 1]) : 4);
            while (f >= end) { p++; end = g.a_off[p + 1] - base; }   // f < N: p stays below n_asm
            tb.keys[f] = r.keyed() && f + tb.k <= end ? r.canon() : KM_NONE;
            tb.tags[f] = (uint32_t)f;
            tb.cnt[f] = 0;
            tb.posc[f] = KM_NO_KEY;
        }
    }
}

// pair q of a step of width j: the lower index has bit j clear; its partner is mirrored in the block of 2 j (the first step of a
// merge) or j higher (every other step)
__device__ inline int64_t pair_low(int64_t q, int64_t j) { return ((q & ~(j - 1)) << 1) | (q & (j - 1)); }
__device__ inline int64_t pair_high(int64_t i, int64_t j, bool mirror) { return mirror ? i ^ (2 * j - 1) : i | j; }

// tail == 0: the merges of 2 .. KM_SORT entries, each in full; tail == 1: the steps of width KM_SORT / 2 .. 1 of a wider merge
__global__ __launch_bounds__(AS_THREADS) void k_km_sort_local(void* table, int tail) {
    __shared__ uint64_t s_key[KM_SORT];
    __shared__ uint32_t s_tag[KM_SORT];
    if (!table_ok(table)) return;
    const Table tb = table_of(table);
    for (int64_t base = (int64_t)blockIdx.x * KM_SORT; base < tb.N; base += (int64_t)gridDim.x * KM_SORT) {
        __syncthreads();
        for (int i = threadIdx.x; i < KM_SORT; i += AS_THREADS) {
            const bool in = base + i < tb.N;   // behind the table: infinite entries, which never move
            s_key[i] = in ? tb.keys[base + i] : KM_NONE;
            s_tag[i] = in ? tb.tags[base + i] : ~0u;
        }
        __syncthreads();
        for (int k = tail ? KM_SORT : 2; k <= KM_SORT; k <<= 1) {
            for (int j = k >> 1; j >= 1; j >>= 1) {
                const bool mirror = !tail && j == (k >> 1);
                for (int q = threadIdx.x; q < KM_SORT / 2; q += AS_THREADS) {
                    const int i = (int)pair_low(q, j), l = (int)pair_high(i, j, mirror);
                    const uint64_t ki = s_key[i], kl = s_key[l];
                    if (kl < ki) {
                        const uint32_t ti = s_tag[i];
                        s_key[i] = kl; s_tag[i] = s_tag[l]; s_key[l] = ki; s_tag[l] = ti;
                    }
                }
                __syncthreads();
            }
        }
        for (int i = threadIdx.x; i < KM_SORT; i += AS_THREADS)
            if (base + i < tb.N) { tb.keys[base + i] = s_key[i]; tb.tags[base + i] = s_tag[i]; }
    }
}

// one step of width j >= KM_SORT: a lane per pair, in global memory
__global__ __launch_bounds__(AS_THREADS) void k_km_sort_global(void* table, int64_t j, int mirror) {
    if (!table_ok(table)) return;
    const Table tb = table_of(table);
    for (int64_t q = (int64_t)blockIdx.x * AS_THREADS + threadIdx.x;; q += (int64_t)gridDim.x * AS_THREADS) {
        const int64_t i = pair_low(q, j), l = pair_high(i, j, mirror);
        if (i >= tb.N) break;   // (i grows with q)
        if (l >= tb.N) continue;
        const uint64_t ki = tb.keys[i], kl = tb.keys[l];
        if (kl < ki) {
            const uint32_t ti = tb.tags[i];
            tb.keys[i] = kl; tb.tags[i] = tb.tags[l]; tb.keys[l] = ki; tb.tags[l] = ti;
        }
    }
}

// the first e in [lo, hi) with keys[e] >= key, or hi
__device__ inline int64_t first_at_least(const uint64_t* keys, int64_t lo, int64_t hi, uint64_t key) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the directory indexes the key's own top bits: bucket b holds the keys in [b << shift, (b + 1) << shift), shift = 2 k - 12
__global__ __launch_bounds__(AS_THREADS) void k_km_dir(BuildArgs g) {
    if (!table_ok(g.table)) return;
    const Table tb = table_of(g.table);
    const int b = blockIdx.x * AS_THREADS + threadIdx.x;
    if (b > KM_DIR) return;
    const uint32_t e = (uint32_t)first_at_least(tb.keys, 0, tb.N, (uint64_t)b << tb.shift);
    tb.dir[b] = e;
    if (b == KM_DIR) { head_of(g.table)[H_KEYED] = e; g.counts[0] = e; }   // every key lies below 1 << 2 k, KM_NONE above
}

// the status is known to the host alone (nothing to build, a table that cannot hold even its head)
__global__ void k_km_build_finish(BuildArgs g, int64_t status, int64_t need, int write_head) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (write_head) {
        int64_t* h = head_of(g.table);
        h[H_MAGIC] = KM_MAGIC; h[H_K] = g.k; h[H_CAP] = g.cap; h[H_NASM] = 0; h[H_N] = 0; h[H_STATUS] = status; h[H_KEYED] = 0;
    }
    g.counts[0] = 0; g.counts[1] = status; g.counts[2] = -1; g.counts[3] = need;
}

// ---- the pass over the reads ------------------------------------------------------------------------------------------------
struct CountArgs { void* table; const uint8_t* bases; const int64_t* base_off; int64_t n_reads, n_bases; };

__global__ __launch_bounds__(AS_THREADS) void k_km_count(CountArgs g) {
    __shared__ uint8_t s_code[KM_TILE + KM_HALO];
    __shared__ uint32_t s_dir[KM_DIR + 1];
    if (!table_ok(g.table)) return;
    const Table tb = table_of(g.table);
    const int64_t keyed = head_of(g.table)[H_KEYED];
    // the reads' bytes [lo, hi): nothing outside the caller's n_bases is read, whatever the offsets hold
    const int64_t lo = max(g.base_off[0], (int64_t)0), hi = min(g.base_off[g.n_reads], g.n_bases);
    if (keyed == 0 || lo + (int64_t)blockIdx.x * KM_TILE >= hi) return;
    const int k = tb.k;
    for (int b = threadIdx.x; b <= KM_DIR; b += AS_THREADS) s_dir[b] = tb.dir[b];
    for (int64_t g0 = lo + (int64_t)blockIdx.x * KM_TILE; g0 < hi; g0 += (int64_t)gridDim.x * KM_TILE) {
        __syncthreads();   // the previous tile has been read
        for (int i = threadIdx.x; i < KM_TILE + k - 1; i += AS_THREADS) s_code[i] = g0 + i < hi ? code_of(g.bases[g0 + i]) : 4;
        __syncthreads();
        const int i0 = threadIdx.x * KM_PER;
        if (g0 + i0 >= hi) continue;
        // the read of the lane's first offset, then forward from it: a k-mer lies inside one read
        int64_t t = owner_of(g.base_off, g.n_reads, g0 + i0);
        int64_t end = g.base_off[t + 1];
        Roll r(k);
        for (int q = 0; q < k - 1; q++) r.push(s_code[i0 + q]);
        for (int m = 0; m < KM_PER; m++) {
            r.push(s_code[i0 + k - 1 + m]);
            const int64_t pos = g0 + i0 + m;
            if (pos >= hi) break;
            while (pos >= end && t + 1 < g.n_reads) { t++; end = g.base_off[t + 1]; }
            if (!r.keyed() || pos + k > end) continue;   // a byte that is no base, or the k bytes are not all in one read
            const uint64_t key = r.canon();
            const uint32_t b = (uint32_t)(key >> tb.shift);
            const int64_t top = s_dir[b + 1], e = first_at_least(tb.keys, s_dir[b], top, key);
            if (e >= top || tb.keys[e] != key) continue;
            // a counter at the cap is left alone, so it cannot wrap: the overshoot is bounded by the lanes in flight
            if (__hip_atomic_load(&tb.cnt[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < tb.cap) atomicAdd(&tb.cnt[e], 1u);
        }
    }
}

// ---- the summary ------------------------------------------------------------------------------------------------------------
struct SupArgs {
    void* table; const int64_t* a_off; int64_t n_asm;
    int64_t min_count; int segment;
    int64_t* ctg;       // [n_asm][3] {keyed, unsupported, without a key}
    int64_t* seg_off;   // [n_asm + 1]
    int64_t seg_capacity; int64_t* segs;
    int64_t run_capacity; int64_t* runs;   // [run_capacity][3] {contig, first, last}
    int64_t* hist;      // [PV_KMER_HIST]
    uint32_t* plane;    // optional, by flat position
    int64_t* counts;    // {runs written, status, runs needed, segment slots needed, summed length or 0, 0, 0, 0}
};

__device__ inline int64_t positions_of(int64_t n, int k) { return n >= k ? n - k + 1 : 0; }

__global__ __launch_bounds__(AS_THREADS) void k_km_sup_setup(SupArgs g) {
    __shared__ int64_t lds[AS_THREADS / 64];
    __shared__ int s_bad;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    for (int64_t p = threadIdx.x; p < g.n_asm; p += AS_THREADS)
        if (g.a_off[p + 1] < g.a_off[p]) s_bad = 1;
    __syncthreads();
    const bool bad = s_bad != 0;
    const int64_t L = bad || g.n_asm == 0 ? 0 : g.a_off[g.n_asm] - g.a_off[0];
    const int64_t* h = head_of(g.table);
    const bool fits = !bad && table_ok(g.table) && h[H_NASM] == g.n_asm && h[H_N] == L && g.min_count <= h[H_CAP];
    const int64_t seg = g.segment;
    const int64_t S = block_scan_to(g.n_asm, g.seg_off, lds, [&](int64_t p) {
        return bad ? (int64_t)0 : (g.a_off[p + 1] - g.a_off[p] + seg - 1) / seg;
    });
    for (int64_t i = threadIdx.x; i < 3 * g.n_asm; i += AS_THREADS) g.ctg[i] = 0;
    for (int i = threadIdx.x; i < PV_KMER_HIST; i += AS_THREADS) g.hist[i] = 0;
    if (threadIdx.x == 0) {
        g.counts[0] = 0;
        g.counts[1] = !fits ? PV_ERR_INVALID : S > g.seg_capacity ? PV_ERR_LIMIT : PV_OK;
        g.counts[2] = 0; g.counts[3] = S; g.counts[4] = L < (1ll << 31) ? L : 0;
        g.counts[5] = g.counts[6] = g.counts[7] = 0;
    }
}

__global__ __launch_bounds__(AS_THREADS) void k_km_gather(SupArgs g) {
    if (g.counts[1] != PV_OK) return;
    const Table tb = table_of(g.table);
    for (int64_t e = (int64_t)blockIdx.x * AS_THREADS + threadIdx.x; e < tb.N; e += (int64_t)gridDim.x * AS_THREADS) {
        const uint64_t key = tb.keys[e];
        uint32_t c = KM_NO_KEY;
        if (key != KM_NONE) {
            const uint32_t b = (uint32_t)(key >> tb.shift);
            const int64_t first = e > 0 && tb.keys[e - 1] == key ? first_at_least(tb.keys, tb.dir[b], e, key) : e;
            c = min(tb.cnt[first], tb.cap);
        }
        const uint32_t f = tb.tags[e];
        tb.posc[f] = c;
        if (g.plane) g.plane[f] = c;
    }
}

__global__ __launch_bounds__(AS_THREADS) void k_km_sums(SupArgs g) {
    __shared__ uint32_t s_hist[PV_KMER_HIST];
    __shared__ int64_t lds[AS_THREADS / 64];
    if (g.counts[1] != PV_OK) return;
    const Table tb = table_of(g.table);
    const int64_t S = g.seg_off[g.n_asm], base = g.a_off[0];
    for (int64_t s = blockIdx.x; s < S; s += gridDim.x) {
        __syncthreads();
        for (int i = threadIdx.x; i < PV_KMER_HIST; i += AS_THREADS) s_hist[i] = 0;
        __syncthreads();
        const int64_t p = owner_of(g.seg_off, g.n_asm, s);
        const int64_t n = g.a_off[p + 1] - g.a_off[p], i0 = (s - g.seg_off[p]) * g.segment;
        const int64_t i1 = min(positions_of(n, tb.k), i0 + g.segment), f0 = g.a_off[p] - base;
        int64_t keyed = 0, unsup = 0;
        for (int64_t i = i0 + threadIdx.x; i < i1; i += AS_THREADS) {
            const uint32_t c = tb.posc[f0 + i];
            if (c == KM_NO_KEY) continue;
            keyed++;
            unsup += c < g.min_count;
            atomicAdd(&s_hist[min(c, (uint32_t)(PV_KMER_HIST - 1))], 1u);
        }
        keyed = block_sum(keyed, lds);
        unsup = block_sum(unsup, lds);   // (its barriers: the LDS histogram is complete)
        if (threadIdx.x == 0) {
            g.segs[s] = unsup;
            atomicAdd((unsigned long long*)&g.ctg[3 * p], (unsigned long long)keyed);
            atomicAdd((unsigned long long*)&g.ctg[3 * p + 1], (unsigned long long)unsup);
        }
        for (int i = threadIdx.x; i < PV_KMER_HIST; i += AS_THREADS)
            if (s_hist[i]) atomicAdd((unsigned long long*)&g.hist[i], (unsigned long long)s_hist[i]);
    }
}

// The last k - 1 bytes of a contig start no k-mer, so they have no key: a run never reaches across a contig's end, and the
// flags need no look at the offsets.
__device__ inline bool unsupported(const Table& tb, int64_t f, int64_t min_count) {
    if (f < 0 || f >= tb.N) return false;
    const uint32_t c = tb.posc[f];
    return c != KM_NO_KEY && c < min_count;
}
// of the lane's KM_RUN_PER positions from f0: bit m set where a run starts (ends) at f0 + m
__device__ inline void run_flags(const Table& tb, int64_t f0, int64_t min_count, uint32_t* starts, uint32_t* ends) {
    uint32_t u = 0;   // bit m + 1: position f0 + m is unsupported
    for (int m = -1; m <= KM_RUN_PER; m++) u |= (uint32_t)unsupported(tb, f0 + m, min_count) << (m + 1);
    const uint32_t own = (u >> 1) & ((1u << KM_RUN_PER) - 1);
    *starts = own & ~u;
    *ends = own & ~(u >> 2);
}

__global__ __launch_bounds__(AS_THREADS) void k_km_run_count(SupArgs g) {
    __shared__ int64_t lds[AS_THREADS / 64];
    if (g.counts[1] != PV_OK) return;
    const Table tb = table_of(g.table);
    const int64_t T = run_tiles(tb.N);
    for (int64_t t = blockIdx.x; t < T; t += gridDim.x) {
        uint32_t st, en;
        run_flags(tb, t * KM_RUN_TILE + (int64_t)threadIdx.x * KM_RUN_PER, g.min_count, &st, &en);
        const int64_t ns = block_sum(__popc(st), lds), ne = block_sum(__popc(en), lds);
        if (threadIdx.x == 0) { tb.tile_cs[t] = ns; tb.tile_ce[t] = ne; }
    }
}

__global__ __launch_bounds__(AS_THREADS) void k_km_run_scan(SupArgs g) {
    __shared__ int64_t lds[AS_THREADS / 64];
    if (g.counts[1] != PV_OK) return;
    const Table tb = table_of(g.table);
    const int64_t T = run_tiles(tb.N);
    const int64_t R = block_scan_to(T, tb.tile_s, lds, [&](int64_t t) { return tb.tile_cs[t]; });
    block_scan_to(T, tb.tile_e, lds, [&](int64_t t) { return tb.tile_ce[t]; });
    for (int64_t p = threadIdx.x; p < g.n_asm; p += AS_THREADS)
        g.ctg[3 * p + 2] = positions_of(g.a_off[p + 1] - g.a_off[p], tb.k) - g.ctg[3 * p];
    if (threadIdx.x == 0) {
        g.counts[2] = R;
        if (R > g.run_capacity) g.counts[1] = PV_ERR_CAPACITY; else g.counts[0] = R;
    }
}

__global__ __launch_bounds__(AS_THREADS) void k_km_run_write(SupArgs g) {
    __shared__ int64_t lds_s[AS_THREADS / 64], lds_e[AS_THREADS / 64];
    if (g.counts[1] != PV_OK) return;
    const Table tb = table_of(g.table);
    const int64_t T = run_tiles(tb.N), base = g.a_off[0];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int64_t t = blockIdx.x; t < T; t += gridDim.x) {
        __syncthreads();   // the previous tile's sums have been read
        if (tb.tile_cs[t] == 0 && tb.tile_ce[t] == 0) continue;
        const int64_t f0 = t * KM_RUN_TILE + (int64_t)threadIdx.x * KM_RUN_PER;
        uint32_t st, en;
        run_flags(tb, f0, g.min_count, &st, &en);
        // exclusive offsets of the lane's starts and ends inside the tile
        int64_t xs = __popc(st), xe = __popc(en);
        const int64_t own_s = xs, own_e = xe;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t ys = __shfl_up(xs, d, 64), ye = __shfl_up(xe, d, 64);
            if (lane >= d) { xs += ys; xe += ye; }
        }
        if (lane == 63) { lds_s[w] = xs; lds_e[w] = xe; }
        __syncthreads();
        int64_t js = tb.tile_s[t] + xs - own_s, je = tb.tile_e[t] + xe - own_e;
        for (int i = 0; i < w; i++) { js += lds_s[i]; je += lds_e[i]; }
        if (st) {
            int64_t p = owner_of(g.a_off, g.n_asm, base + f0);
            for (int m = 0; m < KM_RUN_PER; m++) {
                if (!(st >> m & 1)) continue;
                while (base + f0 + m >= g.a_off[p + 1]) p++;   // a start is a position of a contig: p stays below n_asm
                g.runs[3 * js] = p;
                g.runs[3 * js + 1] = base + f0 + m - g.a_off[p];
                js++;
            }
        }
        if (en) {
            int64_t p = owner_of(g.a_off, g.n_asm, base + f0);
            for (int m = 0; m < KM_RUN_PER; m++) {
                if (!(en >> m & 1)) continue;
                while (base + f0 + m >= g.a_off[p + 1]) p++;
                g.runs[3 * je + 2] = base + f0 + m - g.a_off[p];
                je++;
            }
        }
    }
}

// status < 0: the device's own (counts[1]); else the host's, which also sets the counts
__global__ __launch_bounds__(AS_THREADS) void k_km_poison(SupArgs g, int64_t status, int64_t plane_len) {
    const int64_t t = (int64_t)blockIdx.x * AS_THREADS + threadIdx.x, step = (int64_t)gridDim.x * AS_THREADS;
    if (status != PV_OK && t == 0) {
        g.counts[0] = 0; g.counts[1] = status; g.counts[2] = 0; g.counts[3] = 0;
        g.counts[4] = g.counts[5] = g.counts[6] = g.counts[7] = 0;
    }
    const int64_t st = status != PV_OK ? status : g.counts[1];
    if (st == PV_OK || st == PV_ERR_CAPACITY) return;
    const int64_t L = status != PV_OK ? plane_len : g.counts[4];
    for (int64_t i = t; i < 3 * g.n_asm; i += step) g.ctg[i] = -1;
    for (int64_t i = t; i < g.n_asm + 1; i += step) g.seg_off[i] = -1;
    for (int64_t i = t; i < g.seg_capacity; i += step) g.segs[i] = -1;
    for (int64_t i = t; i < 3 * g.run_capacity; i += step) g.runs[i] = -1;
    for (int64_t i = t; i < PV_KMER_HIST; i += step) g.hist[i] = -1;
    if (g.plane)
        for (int64_t i = t; i < L; i += step) g.plane[i] = KM_NO_KEY;
}

// ---- the reads' k-mers that the assembly lacks (--completeness) ----------------------------------------------------------------
// the reads-only table: head int64 [32] {magic, slots, cap, status, dropped}, keys uint64 [slots], cnt uint32 [slots]
constexpr int64_t KR_MAGIC = 0x5651524D4B5652ll;
constexpr int KR_PROBES = PV_KMER_READS_PROBES;
enum { R_MAGIC, R_SLOTS, R_CAP, R_STATUS, R_DROPPED };

struct Reads { int64_t slots; uint32_t cap; uint64_t* keys; uint32_t* cnt; int64_t* head; };
__host__ __device__ inline bool slots_ok(int64_t s) {
    return s >= PV_KMER_READS_MIN_SLOTS && s <= PV_KMER_READS_MAX_SLOTS && (s & (s - 1)) == 0;
}
__host__ __device__ inline int64_t reads_bytes(int64_t slots) { return KM_HEAD + slots * 12; }
// initialised, and no larger than the memory the caller says it has
__device__ inline bool reads_ok(const void* rtable, int64_t rtable_bytes) {
    const int64_t* h = (const int64_t*)rtable;
    return h[R_MAGIC] == KR_MAGIC && slots_ok(h[R_SLOTS]) && reads_bytes(h[R_SLOTS]) <= rtable_bytes && h[R_CAP] >= 1 &&
           h[R_CAP] <= PV_KMER_MAX_CAP;
}
__device__ inline Reads reads_of(void* rtable) {
    int64_t* h = (int64_t*)rtable;
    uint8_t* b = (uint8_t*)rtable;
    return {h[R_SLOTS], (uint32_t)h[R_CAP], (uint64_t*)(b + KM_HEAD), (uint32_t*)(b + KM_HEAD + h[R_SLOTS] * 8), h};
}

// the splitmix64 finaliser: its low bits choose the home slot, bits 32.. the part
__host__ __device__ inline uint64_t km_mix(uint64_t x) {
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

__global__ __launch_bounds__(AS_THREADS) void k_kr_init(void* rtable, int64_t slots, int64_t cap) {
    uint64_t* keys = (uint64_t*)((uint8_t*)rtable + KM_HEAD);
    uint32_t* cnt = (uint32_t*)((uint8_t*)rtable + KM_HEAD + slots * 8);
    const int64_t t = (int64_t)blockIdx.x * AS_THREADS + threadIdx.x;
    for (int64_t s = t; s < slots; s += (int64_t)gridDim.x * AS_THREADS) { keys[s] = KM_NONE; cnt[s] = 0; }
    if (t < KM_HEAD / 8) {
        int64_t* h = (int64_t*)rtable;
        h[t] = t == R_MAGIC ? KR_MAGIC : t == R_SLOTS ? slots : t == R_CAP ? cap : 0;   // status PV_OK, nothing dropped
    }
}

struct CountAllArgs {
    void* table; void* rtable; int64_t rtable_bytes;
    const uint8_t* bases; const int64_t* base_off; int64_t n_reads, n_bases;
    uint32_t part, n_parts;
};

// k_km_count's tile, halo and directory staging; an instance of another part is passed over, a hit adds to the assembly table
// as there, and a miss goes to the reads-only table: THE HOT PATH with noisy reads, where most instances are misses
__global__ __launch_bounds__(AS_THREADS) void k_km_count_all(CountAllArgs g) {
    __shared__ uint8_t s_code[KM_TILE + KM_HALO];
    __shared__ uint32_t s_dir[KM_DIR + 1];
    if (!table_ok(g.table) || !reads_ok(g.rtable, g.rtable_bytes)) return;
    const Table tb = table_of(g.table);
    const Reads rd = reads_of(g.rtable);
    const bool look = head_of(g.table)[H_KEYED] != 0;   // a table without a key has no directory: every instance is a miss
    const int64_t lo = max(g.base_off[0], (int64_t)0), hi = min(g.base_off[g.n_reads], g.n_bases);
    if (lo + (int64_t)blockIdx.x * KM_TILE >= hi) return;
    const int k = tb.k;
    const uint64_t mask = (uint64_t)rd.slots - 1;
    if (look)
        for (int b = threadIdx.x; b <= KM_DIR; b += AS_THREADS) s_dir[b] = tb.dir[b];
    int64_t dropped = 0;
    bool full = false;
    for (int64_t g0 = lo + (int64_t)blockIdx.x * KM_TILE; g0 < hi; g0 += (int64_t)gridDim.x * KM_TILE) {
        __syncthreads();   // the previous tile has been read
        for (int i = threadIdx.x; i < KM_TILE + k - 1; i += AS_THREADS) s_code[i] = g0 + i < hi ? code_of(g.bases[g0 + i]) : 4;
        __syncthreads();
        // once per tile: after an overflow nothing is probed any more
        full = full || __hip_atomic_load(&rd.head[R_STATUS], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != PV_OK;
        const int i0 = threadIdx.x * KM_PER;
        if (g0 + i0 >= hi) continue;
        int64_t t = owner_of(g.base_off, g.n_reads, g0 + i0);
        int64_t end = g.base_off[t + 1];
        Roll r(k);
        for (int q = 0; q < k - 1; q++) r.push(s_code[i0 + q]);
        for (int m = 0; m < KM_PER; m++) {
            r.push(s_code[i0 + k - 1 + m]);
            const int64_t pos = g0 + i0 + m;
            if (pos >= hi) break;
            while (pos >= end && t + 1 < g.n_reads) { t++; end = g.base_off[t + 1]; }
            if (!r.keyed() || pos + k > end) continue;
            const uint64_t key = r.canon(), h = km_mix(key);
            if (g.n_parts > 1 && (uint32_t)(h >> 32) % g.n_parts != g.part) continue;
            if (look) {
                const uint32_t b = (uint32_t)(key >> tb.shift);
                const int64_t top = s_dir[b + 1], e = first_at_least(tb.keys, s_dir[b], top, key);
                if (e < top && tb.keys[e] == key) {
                    if (__hip_atomic_load(&tb.cnt[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < tb.cap) atomicAdd(&tb.cnt[e], 1u);
                    continue;
                }
            }
            if (full) { dropped++; continue; }
            // a slot's key is written once and stays: a key seen there is final, and only an empty slot needs the compare-and-swap
            uint64_t s = h & mask;
            bool placed = false;
            for (int p = 0; p < KR_PROBES; p++, s = (s + 1) & mask) {
                uint64_t old = __hip_atomic_load(&rd.keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (old == KM_NONE) old = atomicCAS((unsigned long long*)&rd.keys[s], (unsigned long long)KM_NONE, (unsigned long long)key);
                if (old != KM_NONE && old != key) continue;
                if (__hip_atomic_load(&rd.cnt[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < rd.cap) atomicAdd(&rd.cnt[s], 1u);
                placed = true;
                break;
            }
            if (!placed) {
                full = true;
                dropped++;
                __hip_atomic_store(&rd.head[R_STATUS], (int64_t)PV_ERR_CAPACITY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    dropped = wave_sum(dropped);
    if ((threadIdx.x & 63) == 0 && dropped) atomicAdd((unsigned long long*)&rd.head[R_DROPPED], (unsigned long long)dropped);
}

struct FlushArgs { void* rtable; int64_t rtable_bytes; int64_t* ro_hist; int64_t* counts; };

__global__ void k_kr_flush_setup(FlushArgs g) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const bool ok = reads_ok(g.rtable, g.rtable_bytes);
    int64_t* h = (int64_t*)g.rtable;
    g.counts[0] = 0; g.counts[1] = ok ? h[R_STATUS] : PV_ERR_INVALID; g.counts[2] = ok ? h[R_DROPPED] : 0; g.counts[3] = ok ? h[R_SLOTS] : 0;
    if (ok) { h[R_STATUS] = PV_OK; h[R_DROPPED] = 0; }
}

// a lane per slot; the histogram in LDS, flushed by at most 256 atomic adds per workgroup
__global__ __launch_bounds__(AS_THREADS) void k_kr_flush(FlushArgs g) {
    __shared__ uint32_t s_hist[PV_KMER_HIST];
    __shared__ int64_t lds[AS_THREADS / 64];
    if (g.counts[1] == PV_ERR_INVALID) return;
    const Reads rd = reads_of(g.rtable);
    const bool add = g.counts[1] == PV_OK;
    for (int i = threadIdx.x; i < PV_KMER_HIST; i += AS_THREADS) s_hist[i] = 0;
    __syncthreads();
    int64_t n = 0;
    for (int64_t s = (int64_t)blockIdx.x * AS_THREADS + threadIdx.x; s < rd.slots; s += (int64_t)gridDim.x * AS_THREADS) {
        if (rd.keys[s] == KM_NONE) continue;
        n++;
        if (add) atomicAdd(&s_hist[min(min(rd.cnt[s], rd.cap), (uint32_t)(PV_KMER_HIST - 1))], 1u);
        rd.keys[s] = KM_NONE;
        rd.cnt[s] = 0;
    }
    n = block_sum(n, lds);   // (its barriers: the LDS histogram is complete)
    if (threadIdx.x == 0 && n) atomicAdd((unsigned long long*)&g.counts[0], (unsigned long long)n);
    for (int i = threadIdx.x; i < PV_KMER_HIST; i += AS_THREADS)
        if (s_hist[i]) atomicAdd((unsigned long long*)&g.ro_hist[i], (unsigned long long)s_hist[i]);
}

struct SpecArgs { void* table; int64_t* spectrum; int64_t* counts; };

__global__ void k_km_spec_setup(SpecArgs g) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    g.counts[0] = 0; g.counts[1] = table_ok(g.table) ? PV_OK : PV_ERR_INVALID;
}

// a lane per sorted entry: the first of equal keys walks forward over at most three more (only min(m, 4) is asked for)
__global__ __launch_bounds__(AS_THREADS) void k_km_spectrum(SpecArgs g) {
    __shared__ uint32_t s_spec[4 * PV_KMER_HIST];
    __shared__ int64_t lds[AS_THREADS / 64];
    if (g.counts[1] != PV_OK) return;
    const Table tb = table_of(g.table);
    const int64_t keyed = head_of(g.table)[H_KEYED];
    for (int i = threadIdx.x; i < 4 * PV_KMER_HIST; i += AS_THREADS) s_spec[i] = 0;
    __syncthreads();
    int64_t n = 0;
    for (int64_t e = (int64_t)blockIdx.x * AS_THREADS + threadIdx.x; e < keyed; e += (int64_t)gridDim.x * AS_THREADS) {
        const uint64_t key = tb.keys[e];
        if (e > 0 && tb.keys[e - 1] == key) continue;
        int m = 1;
        while (m < 4 && e + m < keyed && tb.keys[e + m] == key) m++;
        const uint32_t c = min(min(tb.cnt[e], tb.cap), (uint32_t)(PV_KMER_HIST - 1));
        atomicAdd(&s_spec[(m - 1) * PV_KMER_HIST + c], 1u);
        n++;
    }
    n = block_sum(n, lds);   // (its barriers: the LDS spectrum is complete)
    if (threadIdx.x == 0 && n) atomicAdd((unsigned long long*)&g.counts[0], (unsigned long long)n);
    for (int i = threadIdx.x; i < 4 * PV_KMER_HIST; i += AS_THREADS)
        if (s_spec[i]) atomicAdd((unsigned long long*)&g.spectrum[i], (unsigned long long)s_spec[i]);
}

unsigned blocks_for(int64_t items, int64_t per_block, int64_t most) {
    return (unsigned)std::max<int64_t>(1, std::min(most, (items + per_block - 1) / per_block));
}

int build_check(int64_t n_asm, int k, int64_t cap) {
    PV_CHECK(n_asm >= 0, PV_ERR_INVALID, "kmer table: negative sizes");
    PV_CHECK(n_asm < (1ll << 31), PV_ERR_LIMIT, "kmer table: too many contigs");
    PV_CHECK(k >= PV_KMER_MIN_K && k <= PV_KMER_MAX_K && (k & 1), PV_ERR_INVALID, "kmer table: k must be odd in [%d, %d] (got %d)",
             PV_KMER_MIN_K, PV_KMER_MAX_K, k);
    PV_CHECK(cap >= 1 && cap <= PV_KMER_MAX_CAP, PV_ERR_INVALID, "kmer table: cap must lie in [1, 2^30] (got %lld)", (long long)cap);
    return PV_OK;
}

int support_check(int64_t n_asm, int64_t min_count, int segment, int64_t seg_capacity, int64_t run_capacity) {
    PV_CHECK(n_asm >= 0 && seg_capacity >= 0 && run_capacity >= 0, PV_ERR_INVALID, "kmer support: negative sizes");
    PV_CHECK(n_asm < (1ll << 31), PV_ERR_LIMIT, "kmer support: too many contigs");
    PV_CHECK(min_count >= 1 && min_count <= PV_KMER_MAX_CAP, PV_ERR_INVALID, "kmer support: min_count must lie in [1, 2^30] (got %lld)",
             (long long)min_count);
    PV_CHECK(segment >= 32 && segment <= 65536 && segment % 32 == 0, PV_ERR_INVALID,
             "kmer support: segment must be a multiple of 32 in [32, 65536] (got %d)", segment);
    return PV_OK;
}

}  // namespace

extern "C" int64_t pv_kmer_table_bytes(int64_t n_asm, const int64_t* a_off) {
    if (n_asm < 0 || (n_asm > 0 && !a_off)) return PV_ERR_INVALID;
    for (int64_t p = 0; p < n_asm; p++)
        if (a_off[p + 1] < a_off[p]) return PV_ERR_INVALID;
    return km_layout(n_asm ? a_off[n_asm] - a_off[0] : 0).total;
}

extern "C" int pv_kmer_table_build_dev(pv_ctx* ctx, const uint8_t* A, const int64_t* a_off, int64_t n_asm, int k, int64_t cap,
                                       void* table, int64_t table_bytes, int64_t* d_counts, void* stream) {
    PV_CHECK(ctx && d_counts, PV_ERR_INVALID, "kmer table: null argument");
    PV_CHECK(table_bytes >= 0 && (table_bytes == 0 || table), PV_ERR_INVALID, "kmer table: table missing");
    int rc;
    if ((rc = build_check(n_asm, k, cap))) return rc;
    PV_CHECK(n_asm == 0 || (A && a_off), PV_ERR_INVALID, "kmer table: sequences or offsets missing");
    PV_CHECK(((uintptr_t)table & 255) == 0, PV_ERR_INVALID, "kmer table: the table must be aligned to 256 bytes");
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = pv_pick_stream(ctx, stream);
    pv_prof_scope ps_all(ctx, "kmer_table_build", st);
    BuildArgs g = {A, a_off, n_asm, k, cap, table, table_bytes, d_counts};
    const int64_t head = km_layout(0).total;   // the least any table needs
    if (table_bytes < head) {
        k_km_build_finish<<<1, 64, 0, st>>>(g, PV_ERR_LIMIT, head, table_bytes >= KM_HEAD);
        PV_HIP(hipGetLastError());
        pv_set_error("kmer table: a table of %lld bytes cannot hold even its head (%lld bytes)", (long long)table_bytes, (long long)head);
        return PV_ERR_LIMIT;
    }
    if (n_asm == 0) {   // nothing is looked at
        k_km_build_finish<<<1, 64, 0, st>>>(g, PV_OK, head, 1);
        PV_HIP(hipGetLastError());
        return PV_OK;
    }
    // what the table could hold bounds every grid and the sort's depth; the kernels take the true size from the device
    const int64_t entries = positions_bound(table_bytes), wide = 8ll * ctx->num_cu;
    k_km_setup<<<1, AS_THREADS, 0, st>>>(g);
    k_km_keys<<<blocks_for(entries, (int64_t)AS_THREADS * KM_STRETCH, wide), AS_THREADS, 0, st>>>(g);
    {
        pv_prof_scope ps(ctx, "k_km_sort", st);
        const unsigned spans = blocks_for(entries, KM_SORT, wide), pairs = blocks_for(entries / 2, AS_THREADS, wide);
        k_km_sort_local<<<spans, AS_THREADS, 0, st>>>(table, 0);
        for (int64_t w = 2 * KM_SORT; (w >> 1) < entries; w <<= 1) {
            for (int64_t j = w >> 1; j >= KM_SORT; j >>= 1) k_km_sort_global<<<pairs, AS_THREADS, 0, st>>>(table, j, j == (w >> 1));
            k_km_sort_local<<<spans, AS_THREADS, 0, st>>>(table, 1);
        }
    }
    k_km_dir<<<KM_DIR / AS_THREADS + 1, AS_THREADS, 0, st>>>(g);
    PV_HIP(hipGetLastError());
    return PV_OK;
}

extern "C" int pv_kmer_count_reads_dev(pv_ctx* ctx, void* table, int64_t table_bytes, const uint8_t* bases, const int64_t* base_off,
                                       int64_t n_reads, int64_t n_bases, void* stream) {
    PV_CHECK(ctx && table && base_off, PV_ERR_INVALID, "kmer count: null argument");
    PV_CHECK(n_reads >= 0 && n_bases >= 0 && (n_bases == 0 || bases), PV_ERR_INVALID, "kmer count: reads missing or negative sizes");
    PV_CHECK(n_bases < (1ll << 31) && n_reads < (1ll << 31), PV_ERR_LIMIT, "kmer count: a batch holds at most 2^31 - 1 bases");
    PV_CHECK(table_bytes >= km_layout(0).total, PV_ERR_LIMIT, "kmer count: the table of %lld bytes cannot hold its head",
             (long long)table_bytes);
    if (n_reads == 0 || n_bases == 0) return PV_OK;
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = pv_pick_stream(ctx, stream);
    pv_prof_scope ps(ctx, "k_km_count", st);
    CountArgs g = {table, bases, base_off, n_reads, n_bases};
    k_km_count<<<blocks_for(n_bases, KM_TILE, 8ll * ctx->num_cu), AS_THREADS, 0, st>>>(g);
    PV_HIP(hipGetLastError());
    return PV_OK;
}

extern "C" int pv_kmer_support_dev(pv_ctx* ctx, void* table, int64_t table_bytes, const int64_t* a_off, int64_t n_asm,
                                   int64_t min_count, int segment, int64_t* contig_counts, int64_t* seg_off, int64_t seg_capacity,
                                   int64_t* segs, int64_t run_capacity, int64_t* runs, int64_t* hist, uint32_t* pos_counts,
                                   int64_t* d_counts, void* stream) {
    PV_CHECK(ctx && table && d_counts && seg_off && hist && a_off, PV_ERR_INVALID, "kmer support: null argument");
    int rc;
    if ((rc = support_check(n_asm, min_count, segment, seg_capacity, run_capacity))) return rc;
    PV_CHECK((n_asm == 0 || contig_counts) && (seg_capacity == 0 || segs) && (run_capacity == 0 || runs), PV_ERR_INVALID,
             "kmer support: an output is missing");
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = pv_pick_stream(ctx, stream);
    pv_prof_scope ps_all(ctx, "kmer_support", st);
    SupArgs g = {table, a_off, n_asm, min_count, segment, contig_counts, seg_off, seg_capacity, segs, run_capacity, runs, hist,
                 pos_counts, d_counts};
    const int64_t wide = 8ll * ctx->num_cu;
    const int64_t outs = std::max(std::max(3 * n_asm + 1, seg_capacity), std::max<int64_t>(3 * run_capacity, PV_KMER_HIST));
    if (table_bytes < km_layout(0).total) {   // no head to read: the plane's length is unknown and it is left alone
        k_km_poison<<<blocks_for(outs, AS_THREADS, wide), AS_THREADS, 0, st>>>(g, PV_ERR_LIMIT, 0);
        PV_HIP(hipGetLastError());
        pv_set_error("kmer support: the table of %lld bytes cannot hold its head", (long long)table_bytes);
        return PV_ERR_LIMIT;
    }
    const int64_t entries = positions_bound(table_bytes);
    k_km_sup_setup<<<1, AS_THREADS, 0, st>>>(g);
    k_km_gather<<<blocks_for(entries, AS_THREADS, wide), AS_THREADS, 0, st>>>(g);
    k_km_sums<<<blocks_for(std::max<int64_t>(seg_capacity, 1), 1, wide), AS_THREADS, 0, st>>>(g);
    k_km_run_count<<<blocks_for(entries, KM_RUN_TILE, wide), AS_THREADS, 0, st>>>(g);
    k_km_run_scan<<<1, AS_THREADS, 0, st>>>(g);
    k_km_run_write<<<blocks_for(entries, KM_RUN_TILE, wide), AS_THREADS, 0, st>>>(g);
    k_km_poison<<<blocks_for(std::max(outs, entries), AS_THREADS, wide), AS_THREADS, 0, st>>>(g, PV_OK, 0);
    PV_HIP(hipGetLastError());
    return PV_OK;
}

extern "C" int pv_kmer_support(pv_ctx* ctx, const uint8_t* A, const int64_t* a_off, int64_t n_asm, const uint8_t* bases,
                               const int64_t* base_off, int64_t n_reads, int k, int64_t cap, int64_t min_count, int segment,
                               int64_t* contig_counts, int64_t* seg_off, int64_t seg_capacity, int64_t* segs, int64_t run_capacity,
                               int64_t* runs, int64_t* hist, uint32_t* pos_counts, int64_t* counts) {
    PV_CHECK(ctx && counts && seg_off && hist && a_off && base_off, PV_ERR_INVALID, "kmer support: null argument");
    int rc;
    if ((rc = build_check(n_asm, k, cap))) return rc;
    if ((rc = support_check(n_asm, min_count, segment, seg_capacity, run_capacity))) return rc;
    PV_CHECK(n_reads >= 0 && n_reads < (1ll << 31), PV_ERR_INVALID, "kmer support: the number of reads must lie in [0, 2^31)");
    PV_CHECK(n_asm == 0 || (A && contig_counts), PV_ERR_INVALID, "kmer support: sequences or counts missing");
    PV_CHECK((seg_capacity == 0 || segs) && (run_capacity == 0 || runs), PV_ERR_INVALID, "kmer support: an output is missing");
    for (int i = 0; i < 8; i++) counts[i] = 0;
    counts[5] = -1;
    // the offsets size the copies, so they are looked at here first: what the device would report, reported the same way
    for (int64_t p = 0; p < n_asm && counts[5] < 0; p++)
        if (a_off[p + 1] < a_off[p]) counts[5] = p;
    bool reads_bad = base_off[0] != 0;
    for (int64_t r = 0; r < n_reads && !reads_bad; r++) reads_bad = base_off[r + 1] < base_off[r];
    const int64_t N = counts[5] < 0 && n_asm ? a_off[n_asm] : 0;
    const bool too_long = N >= (1ll << 31) || (!reads_bad && base_off[n_reads] >= (1ll << 31));
    if (counts[5] >= 0 || (n_asm && a_off[0] != 0) || reads_bad || too_long) {
        const int status = counts[5] >= 0 || (n_asm && a_off[0] != 0) || reads_bad ? PV_ERR_INVALID : PV_ERR_LIMIT;
        counts[1] = status;
        memset(contig_counts, 0xFF, (size_t)n_asm * 24);
        memset(seg_off, 0xFF, (size_t)(n_asm + 1) * 8);
        memset(segs, 0xFF, (size_t)seg_capacity * 8);
        memset(runs, 0xFF, (size_t)run_capacity * 24);
        memset(hist, 0xFF, PV_KMER_HIST * 8);
        PV_CHECK(counts[5] < 0, PV_ERR_INVALID, "kmer support: the offsets of contig %lld decrease", (long long)counts[5]);
        PV_CHECK(!(n_asm && a_off[0] != 0) && !reads_bad, PV_ERR_INVALID, "kmer support: offsets must start at 0 and not decrease");
        counts[6] = km_layout(1ll << 31).total;
        PV_CHECK(false, PV_ERR_LIMIT, "kmer support: the assembly or the reads hold 2^31 bytes or more");
    }
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t na = (size_t)n_asm, nr = (size_t)n_reads, n_b = (size_t)base_off[n_reads];
    const int64_t need = km_layout(N).total;
    uint8_t *d_a = nullptr, *d_b = nullptr, *d_table = nullptr;
    int64_t *d_ao = nullptr, *d_bo = nullptr, *d_ctg = nullptr, *d_so = nullptr, *d_segs = nullptr, *d_runs = nullptr, *d_hist = nullptr;
    int64_t* d_counts = nullptr;
    uint32_t* d_plane = nullptr;
    if ((rc = pv_get(ctx, "km.a", (size_t)N + 1, &d_a))) return rc;
    if ((rc = pv_get(ctx, "km.b", n_b + 1, &d_b))) return rc;
    if ((rc = pv_get(ctx, "km.a_off", na + 1, &d_ao))) return rc;
    if ((rc = pv_get(ctx, "km.b_off", nr + 1, &d_bo))) return rc;
    if ((rc = pv_get(ctx, "km.table", (size_t)need, &d_table))) return rc;
    if ((rc = pv_get(ctx, "km.ctg", 3 * na + 1, &d_ctg))) return rc;
    if ((rc = pv_get(ctx, "km.seg_off", na + 1, &d_so))) return rc;
    if ((rc = pv_get(ctx, "km.segs", (size_t)seg_capacity + 1, &d_segs))) return rc;
    if ((rc = pv_get(ctx, "km.runs", 3 * (size_t)run_capacity + 1, &d_runs))) return rc;
    if ((rc = pv_get(ctx, "km.hist", (size_t)PV_KMER_HIST, &d_hist))) return rc;
    if ((rc = pv_get(ctx, "km.counts", (size_t)12, &d_counts))) return rc;
    if (pos_counts && (rc = pv_get(ctx, "km.plane", (size_t)N + 1, &d_plane))) return rc;
    if (N) PV_HIP(hipMemcpyAsync(d_a, A, (size_t)N, hipMemcpyHostToDevice, st));
    if (n_b) PV_HIP(hipMemcpyAsync(d_b, bases, n_b, hipMemcpyHostToDevice, st));
    PV_HIP(hipMemcpyAsync(d_ao, a_off, (na + 1) * 8, hipMemcpyHostToDevice, st));
    PV_HIP(hipMemcpyAsync(d_bo, base_off, (nr + 1) * 8, hipMemcpyHostToDevice, st));
    // the caller's run records stay as they were where none is written (PV_ERR_CAPACITY)
    if (run_capacity) PV_HIP(hipMemcpyAsync(d_runs, runs, (size_t)run_capacity * 24, hipMemcpyHostToDevice, st));
    if ((rc = pv_kmer_table_build_dev(ctx, d_a, d_ao, n_asm, k, cap, d_table, need, d_counts + 8, st))) return rc;
    if ((rc = pv_kmer_count_reads_dev(ctx, d_table, need, d_b, d_bo, n_reads, (int64_t)n_b, st))) return rc;
    if ((rc = pv_kmer_support_dev(ctx, d_table, need, d_ao, n_asm, min_count, segment, d_ctg, d_so, seg_capacity, d_segs,
                                  run_capacity, d_runs, d_hist, pos_counts ? d_plane : nullptr, d_counts, st)))
        return rc;
    int64_t h[12];
    PV_HIP(hipMemcpyAsync(h, d_counts, sizeof(h), hipMemcpyDeviceToHost, st));
    if (na) PV_HIP(hipMemcpyAsync(contig_counts, d_ctg, na * 24, hipMemcpyDeviceToHost, st));
    PV_HIP(hipMemcpyAsync(seg_off, d_so, (na + 1) * 8, hipMemcpyDeviceToHost, st));
    if (seg_capacity) PV_HIP(hipMemcpyAsync(segs, d_segs, (size_t)seg_capacity * 8, hipMemcpyDeviceToHost, st));
    if (run_capacity) PV_HIP(hipMemcpyAsync(runs, d_runs, (size_t)run_capacity * 24, hipMemcpyDeviceToHost, st));
    PV_HIP(hipMemcpyAsync(hist, d_hist, PV_KMER_HIST * 8, hipMemcpyDeviceToHost, st));
    if (pos_counts && N) PV_HIP(hipMemcpyAsync(pos_counts, d_plane, (size_t)N * 4, hipMemcpyDeviceToHost, st));
    PV_HIP(hipStreamSynchronize(st));
    counts[0] = h[0]; counts[1] = h[1]; counts[2] = h[2]; counts[3] = h[3];
    counts[4] = h[8]; counts[5] = h[10]; counts[6] = h[11];
    PV_CHECK(counts[1] == PV_OK, (int)counts[1], "kmer support: device status %lld (%lld run records, %lld segment slots needed)",
             (long long)counts[1], (long long)counts[2], (long long)counts[3]);
    return PV_OK;
}

// ---- --completeness: the reads-only table, the count of every part, the flush, the assembly's spectrum -------------------------
namespace {

int reads_check(const void* rtable, int64_t rtable_bytes) {
    PV_CHECK(rtable, PV_ERR_INVALID, "kmer reads table: null argument");
    PV_CHECK(rtable_bytes >= reads_bytes(PV_KMER_READS_MIN_SLOTS), PV_ERR_INVALID,
             "kmer reads table: %lld bytes cannot hold the smallest table (%lld bytes)", (long long)rtable_bytes,
             (long long)reads_bytes(PV_KMER_READS_MIN_SLOTS));
    PV_CHECK(((uintptr_t)rtable & 255) == 0, PV_ERR_INVALID, "kmer reads table: the table must be aligned to 256 bytes");
    return PV_OK;
}
// a bound of the slots a table of `bytes` can hold: it sizes the flush's grid, the kernel takes the slots from the head
inline int64_t slots_bound(int64_t bytes) { return (bytes - KM_HEAD) / 12; }

}  // namespace

extern "C" int64_t pv_kmer_reads_table_bytes(int64_t slots) { return slots_ok(slots) ? reads_bytes(slots) : (int64_t)PV_ERR_INVALID; }

extern "C" int pv_kmer_reads_table_init_dev(pv_ctx* ctx, void* rtable, int64_t rtable_bytes, int64_t slots, int64_t cap, void* stream) {
    PV_CHECK(ctx, PV_ERR_INVALID, "kmer reads table: null argument");
    int rc;
    if ((rc = reads_check(rtable, rtable_bytes))) return rc;
    PV_CHECK(slots_ok(slots), PV_ERR_INVALID, "kmer reads table: slots must be a power of two in [1024, 2^34] (got %lld)", (long long)slots);
    PV_CHECK(reads_bytes(slots) <= rtable_bytes, PV_ERR_INVALID, "kmer reads table: %lld slots need %lld bytes (got %lld)",
             (long long)slots, (long long)reads_bytes(slots), (long long)rtable_bytes);
    PV_CHECK(cap >= 1 && cap <= PV_KMER_MAX_CAP, PV_ERR_INVALID, "kmer reads table: cap must lie in [1, 2^30] (got %lld)", (long long)cap);
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = pv_pick_stream(ctx, stream);
    pv_prof_scope ps(ctx, "k_kr_init", st);
    k_kr_init<<<blocks_for(slots, 4ll * AS_THREADS, 16ll * ctx->num_cu), AS_THREADS, 0, st>>>(rtable, slots, cap);
    PV_HIP(hipGetLastError());
    return PV_OK;
}

extern "C" int pv_kmer_count_reads_all_dev(pv_ctx* ctx, void* table, int64_t table_bytes, void* rtable, int64_t rtable_bytes,
                                           const uint8_t* bases, const int64_t* base_off, int64_t n_reads, int64_t n_bases, int part,
                                           int n_parts, void* stream) {
    PV_CHECK(ctx && table && base_off, PV_ERR_INVALID, "kmer count: null argument");
    int rc;
    if ((rc = reads_check(rtable, rtable_bytes))) return rc;
    PV_CHECK(n_reads >= 0 && n_bases >= 0 && (n_bases == 0 || bases), PV_ERR_INVALID, "kmer count: reads missing or negative sizes");
    PV_CHECK(n_parts >= 1 && n_parts <= PV_KMER_MAX_PARTS && part >= 0 && part < n_parts, PV_ERR_INVALID,
             "kmer count: part %d of %d: the parts must lie in [1, %d] and the part below them", part, n_parts, PV_KMER_MAX_PARTS);
    PV_CHECK(n_bases < (1ll << 31) && n_reads < (1ll << 31), PV_ERR_LIMIT, "kmer count: a batch holds at most 2^31 - 1 bases");
    PV_CHECK(table_bytes >= km_layout(0).total, PV_ERR_LIMIT, "kmer count: the table of %lld bytes cannot hold its head",
             (long long)table_bytes);
    if (n_reads == 0 || n_bases == 0) return PV_OK;
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = pv_pick_stream(ctx, stream);
    pv_prof_scope ps(ctx, "k_km_count_all", st);
    CountAllArgs g = {table, rtable, rtable_bytes, bases, base_off, n_reads, n_bases, (uint32_t)part, (uint32_t)n_parts};
    k_km_count_all<<<blocks_for(n_bases, KM_TILE, 8ll * ctx->num_cu), AS_THREADS, 0, st>>>(g);
    PV_HIP(hipGetLastError());
    return PV_OK;
}

extern "C" int pv_kmer_reads_flush_dev(pv_ctx* ctx, void* rtable, int64_t rtable_bytes, int64_t* ro_hist, int64_t* d_counts,
                                       void* stream) {
    PV_CHECK(ctx && ro_hist && d_counts, PV_ERR_INVALID, "kmer reads flush: null argument");
    int rc;
    if ((rc = reads_check(rtable, rtable_bytes))) return rc;
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = pv_pick_stream(ctx, stream);
    pv_prof_scope ps(ctx, "kmer_reads_flush", st);
    FlushArgs g = {rtable, rtable_bytes, ro_hist, d_counts};
    k_kr_flush_setup<<<1, 64, 0, st>>>(g);
    k_kr_flush<<<blocks_for(slots_bound(rtable_bytes), 4ll * AS_THREADS, 16ll * ctx->num_cu), AS_THREADS, 0, st>>>(g);
    PV_HIP(hipGetLastError());
    return PV_OK;
}

extern "C" int pv_kmer_spectrum_dev(pv_ctx* ctx, void* table, int64_t table_bytes, int64_t* spectrum, int64_t* d_counts, void* stream) {
    PV_CHECK(ctx && table && spectrum && d_counts, PV_ERR_INVALID, "kmer spectrum: null argument");
    PV_CHECK(table_bytes >= km_layout(0).total, PV_ERR_LIMIT, "kmer spectrum: the table of %lld bytes cannot hold its head",
             (long long)table_bytes);
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = pv_pick_stream(ctx, stream);
    pv_prof_scope ps(ctx, "kmer_spectrum", st);
    SpecArgs g = {table, spectrum, d_counts};
    k_km_spec_setup<<<1, 64, 0, st>>>(g);
    k_km_spectrum<<<blocks_for(positions_bound(table_bytes), AS_THREADS, 8ll * ctx->num_cu), AS_THREADS, 0, st>>>(g);
    PV_HIP(hipGetLastError());
    return PV_OK;
}

extern "C" int pv_kmer_spectrum(pv_ctx* ctx, const uint8_t* A, const int64_t* a_off, int64_t n_asm, const uint8_t* bases,
                                const int64_t* base_off, int64_t n_reads, int k, int64_t cap, int64_t slots, int n_parts,
                                int64_t* spectrum, int64_t* ro_hist, int64_t* counts) {
    PV_CHECK(ctx && counts && spectrum && ro_hist && a_off && base_off, PV_ERR_INVALID, "kmer spectrum: null argument");
    int rc;
    if ((rc = build_check(n_asm, k, cap))) return rc;
    PV_CHECK(n_reads >= 0 && n_reads < (1ll << 31), PV_ERR_INVALID, "kmer spectrum: the number of reads must lie in [0, 2^31)");
    PV_CHECK(n_asm == 0 || A, PV_ERR_INVALID, "kmer spectrum: sequences missing");
    PV_CHECK(slots_ok(slots), PV_ERR_INVALID, "kmer spectrum: slots must be a power of two in [1024, 2^34] (got %lld)", (long long)slots);
    PV_CHECK(n_parts >= 1 && n_parts <= PV_KMER_MAX_PARTS, PV_ERR_INVALID, "kmer spectrum: the parts must lie in [1, %d] (got %d)",
             PV_KMER_MAX_PARTS, n_parts);
    for (int i = 0; i < 8; i++) counts[i] = 0;
    bool bad = (n_asm && a_off[0] != 0) || base_off[0] != 0;
    for (int64_t p = 0; p < n_asm && !bad; p++) bad = a_off[p + 1] < a_off[p];
    for (int64_t r = 0; r < n_reads && !bad; r++) bad = base_off[r + 1] < base_off[r];
    if (bad) counts[1] = PV_ERR_INVALID;
    PV_CHECK(!bad, PV_ERR_INVALID, "kmer spectrum: offsets must start at 0 and not decrease");
    const int64_t N = n_asm ? a_off[n_asm] : 0;
    if (N >= (1ll << 31) || base_off[n_reads] >= (1ll << 31)) counts[1] = PV_ERR_LIMIT;
    PV_CHECK(counts[1] == PV_OK, PV_ERR_LIMIT, "kmer spectrum: the assembly or the reads hold 2^31 bytes or more");
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t na = (size_t)n_asm, nr = (size_t)n_reads, n_b = (size_t)base_off[n_reads], np = (size_t)n_parts;
    const int64_t need = km_layout(N).total, rneed = reads_bytes(slots);
    uint8_t *d_a = nullptr, *d_b = nullptr, *d_table = nullptr, *d_rtable = nullptr;
    int64_t *d_ao = nullptr, *d_bo = nullptr, *d_out = nullptr, *d_counts = nullptr;
    if ((rc = pv_get(ctx, "km.a", (size_t)N + 1, &d_a))) return rc;
    if ((rc = pv_get(ctx, "km.b", n_b + 1, &d_b))) return rc;
    if ((rc = pv_get(ctx, "km.a_off", na + 1, &d_ao))) return rc;
    if ((rc = pv_get(ctx, "km.b_off", nr + 1, &d_bo))) return rc;
    if ((rc = pv_get(ctx, "km.table", (size_t)need, &d_table))) return rc;
    if ((rc = pv_get(ctx, "km.rtable", (size_t)rneed, &d_rtable))) return rc;
    if ((rc = pv_get(ctx, "km.spectrum", (size_t)5 * PV_KMER_HIST, &d_out))) return rc;   // the spectrum, then ro_hist
    if ((rc = pv_get(ctx, "km.fcounts", 4 * np + 8, &d_counts))) return rc;                // {build 4, spectrum 2, 0, 0}, a flush's 4 per part
    if (N) PV_HIP(hipMemcpyAsync(d_a, A, (size_t)N, hipMemcpyHostToDevice, st));
    if (n_b) PV_HIP(hipMemcpyAsync(d_b, bases, n_b, hipMemcpyHostToDevice, st));
    PV_HIP(hipMemcpyAsync(d_ao, a_off, (na + 1) * 8, hipMemcpyHostToDevice, st));
    PV_HIP(hipMemcpyAsync(d_bo, base_off, (nr + 1) * 8, hipMemcpyHostToDevice, st));
    if ((rc = pv_zero_async(d_out, (size_t)5 * PV_KMER_HIST * 8, st))) return rc;
    if ((rc = pv_kmer_table_build_dev(ctx, d_a, d_ao, n_asm, k, cap, d_table, need, d_counts, st))) return rc;
    if ((rc = pv_kmer_reads_table_init_dev(ctx, d_rtable, rneed, slots, cap, st))) return rc;
    for (int p = 0; p < n_parts; p++) {
        if ((rc = pv_kmer_count_reads_all_dev(ctx, d_table, need, d_rtable, rneed, d_b, d_bo, n_reads, (int64_t)n_b, p, n_parts, st)))
            return rc;
        if ((rc = pv_kmer_reads_flush_dev(ctx, d_rtable, rneed, d_out + 4 * PV_KMER_HIST, d_counts + 8 + 4 * p, st))) return rc;
    }
    if ((rc = pv_kmer_spectrum_dev(ctx, d_table, need, d_out, d_counts + 4, st))) return rc;
    std::vector<int64_t> h(4 * np + 8);
    PV_HIP(hipMemcpyAsync(h.data(), d_counts, h.size() * 8, hipMemcpyDeviceToHost, st));
    PV_HIP(hipMemcpyAsync(spectrum, d_out, (size_t)4 * PV_KMER_HIST * 8, hipMemcpyDeviceToHost, st));
    PV_HIP(hipMemcpyAsync(ro_hist, d_out + 4 * PV_KMER_HIST, (size_t)PV_KMER_HIST * 8, hipMemcpyDeviceToHost, st));
    PV_HIP(hipStreamSynchronize(st));
    counts[1] = h[1];
    for (size_t p = 0; p < np; p++) {
        counts[0] += h[8 + 4 * p];
        if (counts[1] == PV_OK) counts[1] = h[8 + 4 * p + 1];
        counts[2] += h[8 + 4 * p + 2];
    }
    if (counts[1] == PV_OK) counts[1] = h[5];
    counts[3] = slots; counts[4] = h[0]; counts[5] = h[4];
    PV_CHECK(counts[1] == PV_OK, (int)counts[1], "kmer spectrum: device status %lld (%lld read k-mers dropped from %lld slots)",
             (long long)counts[1], (long long)counts[2], (long long)slots);
    return PV_OK;
}
