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
//     k_km_sort_local   the bitonic sort of kmer_index.hpp (spans of KM_SORT entries in LDS, the wider steps one launch each),
//     k_km_sort_global  ordered by key alone
//     k_km_dir          where the keys of each value of their own top 12 bits (of 2 k) begin, and the number of keyed entries
//   pv_kmer_count_reads_dev
//     k_km_count        THE HOT PATH. The tile walk of kmer_index.hpp over the reads, PV_KMER_TILE bytes and a (k - 1)-byte
//                       halo at a time; its visitor is count_hit: the canonical key of an offset inside one read is found
//                       (directory in LDS, then a binary search in L2) and one is added to the counter of the first entry
//                       with that key, unless it has reached the cap
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
//     k_km_count_all    the same walk with a second visitor: an instance of another part is passed over, count_hit takes the
//                       keys the assembly has, and a key it lacks claims or finds its slot (linear probing from mix(key), one
//                       64-bit compare-and-swap on an empty slot) and adds one there under the cap
//   pv_kmer_reads_flush_dev
//     k_kr_flush_setup  one lane: the head checked, {0, status, dropped, slots}, status and dropped reset
//     k_kr_flush        a lane per slot: the histogram of the counts in LDS, the table emptied
//   pv_kmer_spectrum_dev
//     k_km_spec_setup   one lane: the table's status
//     k_km_spectrum     a lane per sorted entry: the first of equal keys adds its (multiplicity, count) to the spectrum in LDS
// The counters are integer atomics: the result does not depend on tile size, workgroup count or the order of the calls.
#include "kmer_index.hpp"
#include "pv_common.hpp"

namespace {

constexpr int KM_TILE = PV_KMER_TILE;           // a lane of the count takes KM_TILE / AS_THREADS consecutive offsets
constexpr int KM_HALO = PV_KMER_MAX_K - 1;
constexpr int KM_STRETCH = 32;                  // consecutive positions of a lane of the key kernel
constexpr int KM_SORT = PV_KMER_SORT_SPAN;      // entries a workgroup sorts in LDS
constexpr int KM_DIR_BITS = KI_DIR_BITS, KM_DIR = KI_DIR;
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

__global__ __launch_bounds__(AS_THREADS) void k_km_sort_local(void* table, int tail) {
    if (!table_ok(table)) return;
    const Table tb = table_of(table);
    sort_spans<KM_SORT, ByKey>(tb.keys, tb.tags, tb.N, tail);
}

__global__ __launch_bounds__(AS_THREADS) void k_km_sort_global(void* table, int64_t j, int mirror) {
    if (!table_ok(table)) return;
    const Table tb = table_of(table);
    sort_global_step<ByKey>(tb.keys, tb.tags, tb.N, j, mirror);
}

// the directory indexes the key's own top bits: bucket b holds the keys in [b << shift, (b + 1) << shift), shift = 2 k - 12
__global__ __launch_bounds__(AS_THREADS) void k_km_dir(BuildArgs g) {
    if (!table_ok(g.table)) return;
    const Table tb = table_of(g.table);
    const int b = blockIdx.x * AS_THREADS + threadIdx.x;
    if (b > KM_DIR) return;
    const uint32_t e = dir_entry(tb.keys, tb.N, b, tb.shift);
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

// a key the table holds: one more on the counter of the first entry with it; s_dir: the table's directory
__device__ inline bool count_hit(const Table& tb, const uint32_t* s_dir, uint64_t key) {
    const DirHit h = dir_find(s_dir, tb.keys, key, tb.shift);
    if (h.e >= h.top || tb.keys[h.e] != key) return false;
    add_capped(&tb.cnt[h.e], tb.cap);
    return true;
}

__global__ __launch_bounds__(AS_THREADS) void k_km_count(CountArgs g) {
    __shared__ uint8_t s_code[KM_TILE + KM_HALO];
    __shared__ uint32_t s_dir[KM_DIR + 1];
    if (!table_ok(g.table)) return;
    const Table tb = table_of(g.table);
    const int64_t keyed = head_of(g.table)[H_KEYED];
    // the reads' bytes [lo, hi): nothing outside the caller's n_bases is read, whatever the offsets hold
    const int64_t lo = max(g.base_off[0], (int64_t)0), hi = min(g.base_off[g.n_reads], g.n_bases);
    if (keyed == 0 || lo + (int64_t)blockIdx.x * KM_TILE >= hi) return;
    for (int b = threadIdx.x; b <= KM_DIR; b += AS_THREADS) s_dir[b] = tb.dir[b];
    tile_walk<KM_TILE>(g.bases, g.base_off, g.n_reads, lo, hi, tb.k, s_code, [] {},
                       [&](const Roll& r, int64_t, int64_t, int64_t) { count_hit(tb, s_dir, r.canon()); });
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
        keyed = block_reduce(keyed, lds, as_add());
        unsup = block_reduce(unsup, lds, as_add());   // (its barriers: the LDS histogram is complete)
        if (threadIdx.x == 0) {
            g.segs[s] = unsup;
            atomicAdd((unsigned long long*)&g.ctg[3 * p], (unsigned long long)keyed);
            atomicAdd((unsigned long long*)&g.ctg[3 * p + 1], (unsigned long long)unsup);
        }
        lds_hist_flush(s_hist, PV_KMER_HIST, g.hist);
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
        const int64_t ns = block_reduce((int64_t)__popc(st), lds, as_add()), ne = block_reduce((int64_t)__popc(en), lds, as_add());
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
        // put(contig, offset in it) for every set bit of the lane's starts or ends, in order
        const auto each = [&](uint32_t bits, auto put) {
            if (!bits) return;
            int64_t p = owner_of(g.a_off, g.n_asm, base + f0);
            for (int m = 0; m < KM_RUN_PER; m++) {
                if (!(bits >> m & 1)) continue;
                while (base + f0 + m >= g.a_off[p + 1]) p++;   // a set bit is a position of a contig: p stays below n_asm
                put(p, base + f0 + m - g.a_off[p]);
            }
        };
        each(st, [&](int64_t p, int64_t at) { g.runs[3 * js] = p; g.runs[3 * js + 1] = at; js++; });
        each(en, [&](int64_t, int64_t at) { g.runs[3 * je + 2] = at; je++; });
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

// k_km_count's walk and directory; an instance of another part is passed over, a hit adds to the assembly table as there, and
// a miss goes to the reads-only table: THE HOT PATH with noisy reads, where most instances are misses
__global__ __launch_bounds__(AS_THREADS) void k_km_count_all(CountAllArgs g) {
    __shared__ uint8_t s_code[KM_TILE + KM_HALO];
    __shared__ uint32_t s_dir[KM_DIR + 1];
    if (!table_ok(g.table) || !reads_ok(g.rtable, g.rtable_bytes)) return;
    const Table tb = table_of(g.table);
    const Reads rd = reads_of(g.rtable);
    const bool look = head_of(g.table)[H_KEYED] != 0;   // a table without a key has no directory: every instance is a miss
    const int64_t lo = max(g.base_off[0], (int64_t)0), hi = min(g.base_off[g.n_reads], g.n_bases);
    if (lo + (int64_t)blockIdx.x * KM_TILE >= hi) return;
    const uint64_t mask = (uint64_t)rd.slots - 1;
    if (look)
        for (int b = threadIdx.x; b <= KM_DIR; b += AS_THREADS) s_dir[b] = tb.dir[b];
    int64_t dropped = 0;
    bool full = false;
    // once per tile: after an overflow nothing is probed any more
    const auto per_tile = [&] { full = full || __hip_atomic_load(&rd.head[R_STATUS], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != PV_OK; };
    tile_walk<KM_TILE>(g.bases, g.base_off, g.n_reads, lo, hi, tb.k, s_code, per_tile, [&](const Roll& r, int64_t, int64_t, int64_t) {
        const uint64_t key = r.canon(), h = km_mix(key);
        if (g.n_parts > 1 && (uint32_t)(h >> 32) % g.n_parts != g.part) return;
        if (look && count_hit(tb, s_dir, key)) return;
        if (full) { dropped++; return; }
        // a slot's key is written once and stays: a key seen there is final, and only an empty slot needs the compare-and-swap
        uint64_t s = h & mask;
        bool placed = false;   // (a flag, not a return out of the loop, which compiles to twice the compare-and-swap sites)
        for (int p = 0; p < KR_PROBES; p++, s = (s + 1) & mask) {
            uint64_t old = __hip_atomic_load(&rd.keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (old == KM_NONE) old = atomicCAS((unsigned long long*)&rd.keys[s], (unsigned long long)KM_NONE, (unsigned long long)key);
            if (old != KM_NONE && old != key) continue;
            add_capped(&rd.cnt[s], rd.cap);
            placed = true;
            break;
        }
        if (!placed) {
            full = true;
            dropped++;
            __hip_atomic_store(&rd.head[R_STATUS], (int64_t)PV_ERR_CAPACITY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    });
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
    n = block_reduce(n, lds, as_add());   // (its barriers: the LDS histogram is complete)
    if (threadIdx.x == 0 && n) atomicAdd((unsigned long long*)&g.counts[0], (unsigned long long)n);
    lds_hist_flush(s_hist, PV_KMER_HIST, g.ro_hist);
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
    n = block_reduce(n, lds, as_add());   // (its barriers: the LDS spectrum is complete)
    if (threadIdx.x == 0 && n) atomicAdd((unsigned long long*)&g.counts[0], (unsigned long long)n);
    lds_hist_flush(s_spec, 4 * PV_KMER_HIST, g.spectrum);
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

// what both passes over the reads ask of a batch; pv_kmer_count_reads_dev is part 0 of 1
int count_check(int64_t table_bytes, const uint8_t* bases, int64_t n_reads, int64_t n_bases, int part, int n_parts) {
    PV_CHECK(n_reads >= 0 && n_bases >= 0 && (n_bases == 0 || bases), PV_ERR_INVALID, "kmer count: reads missing or negative sizes");
    PV_CHECK(n_parts >= 1 && n_parts <= PV_KMER_MAX_PARTS && part >= 0 && part < n_parts, PV_ERR_INVALID,
             "kmer count: part %d of %d: the parts must lie in [1, %d] and the part below them", part, n_parts, PV_KMER_MAX_PARTS);
    PV_CHECK(n_bases < (1ll << 31) && n_reads < (1ll << 31), PV_ERR_LIMIT, "kmer count: a batch holds at most 2^31 - 1 bases");
    PV_CHECK(table_bytes >= km_layout(0).total, PV_ERR_LIMIT, "kmer count: the table of %lld bytes cannot hold its head",
             (long long)table_bytes);
    return PV_OK;
}

// The host forms' way to the device. The offsets size the copies, so they are looked at first: what the device would report.
// With offsets that are in order (ok()), the assembly, the reads and both offset arrays are on the device, next to a table.
struct Staged {
    int64_t bad_contig = -1;   // the first contig whose offsets decrease
    bool bad_start = false, bad_reads = false, too_long = false;
    int64_t N = 0, need = 0;   // the summed assembly length, the table's bytes
    size_t n_b = 0;            // the reads' bytes
    uint8_t *a = nullptr, *b = nullptr, *table = nullptr;
    int64_t *a_off = nullptr, *b_off = nullptr;
    bool invalid() const { return bad_contig >= 0 || bad_start || bad_reads; }
    bool ok() const { return !invalid() && !too_long; }
};
int km_stage(pv_ctx* ctx, const uint8_t* A, const int64_t* a_off, int64_t n_asm, const uint8_t* bases, const int64_t* base_off,
             int64_t n_reads, Staged* s) {
    for (int64_t p = 0; p < n_asm && s->bad_contig < 0; p++)
        if (a_off[p + 1] < a_off[p]) s->bad_contig = p;
    s->bad_start = n_asm && a_off[0] != 0;
    s->bad_reads = base_off[0] != 0;
    for (int64_t r = 0; r < n_reads && !s->bad_reads; r++) s->bad_reads = base_off[r + 1] < base_off[r];
    s->N = s->bad_contig < 0 && n_asm ? a_off[n_asm] : 0;
    s->too_long = s->N >= (1ll << 31) || (!s->bad_reads && base_off[n_reads] >= (1ll << 31));
    if (!s->ok()) return PV_OK;
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t na = (size_t)n_asm, nr = (size_t)n_reads;
    s->n_b = (size_t)base_off[n_reads];
    s->need = km_layout(s->N).total;
    int rc;
    if ((rc = pv_get(ctx, "km.a", (size_t)s->N + 1, &s->a))) return rc;
    if ((rc = pv_get(ctx, "km.b", s->n_b + 1, &s->b))) return rc;
    if ((rc = pv_get(ctx, "km.a_off", na + 1, &s->a_off))) return rc;
    if ((rc = pv_get(ctx, "km.b_off", nr + 1, &s->b_off))) return rc;
    if ((rc = pv_get(ctx, "km.table", (size_t)s->need, &s->table))) return rc;
    if (s->N) PV_HIP(hipMemcpyAsync(s->a, A, (size_t)s->N, hipMemcpyHostToDevice, st));
    if (s->n_b) PV_HIP(hipMemcpyAsync(s->b, bases, s->n_b, hipMemcpyHostToDevice, st));
    PV_HIP(hipMemcpyAsync(s->a_off, a_off, (na + 1) * 8, hipMemcpyHostToDevice, st));
    PV_HIP(hipMemcpyAsync(s->b_off, base_off, (nr + 1) * 8, hipMemcpyHostToDevice, st));
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
        sort_schedule(entries, KM_SORT, [&](int tail) { k_km_sort_local<<<spans, AS_THREADS, 0, st>>>(table, tail); },
                      [&](int64_t j, int mirror) { k_km_sort_global<<<pairs, AS_THREADS, 0, st>>>(table, j, mirror); });
    }
    k_km_dir<<<KM_DIR / AS_THREADS + 1, AS_THREADS, 0, st>>>(g);
    PV_HIP(hipGetLastError());
    return PV_OK;
}

extern "C" int pv_kmer_count_reads_dev(pv_ctx* ctx, void* table, int64_t table_bytes, const uint8_t* bases, const int64_t* base_off,
                                       int64_t n_reads, int64_t n_bases, void* stream) {
    PV_CHECK(ctx && table && base_off, PV_ERR_INVALID, "kmer count: null argument");
    int rc;
    if ((rc = count_check(table_bytes, bases, n_reads, n_bases, 0, 1))) return rc;
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
    Staged s;
    if ((rc = km_stage(ctx, A, a_off, n_asm, bases, base_off, n_reads, &s))) return rc;
    counts[5] = s.bad_contig;
    if (!s.ok()) {   // reported the way the device reports it
        counts[1] = s.invalid() ? PV_ERR_INVALID : PV_ERR_LIMIT;
        memset(contig_counts, 0xFF, (size_t)n_asm * 24);
        memset(seg_off, 0xFF, (size_t)(n_asm + 1) * 8);
        memset(segs, 0xFF, (size_t)seg_capacity * 8);
        memset(runs, 0xFF, (size_t)run_capacity * 24);
        memset(hist, 0xFF, PV_KMER_HIST * 8);
        PV_CHECK(counts[5] < 0, PV_ERR_INVALID, "kmer support: the offsets of contig %lld decrease", (long long)counts[5]);
        PV_CHECK(!s.bad_start && !s.bad_reads, PV_ERR_INVALID, "kmer support: offsets must start at 0 and not decrease");
        counts[6] = km_layout(1ll << 31).total;
        PV_CHECK(false, PV_ERR_LIMIT, "kmer support: the assembly or the reads hold 2^31 bytes or more");
    }
    hipStream_t st = ctx->stream;
    const size_t na = (size_t)n_asm;
    const int64_t N = s.N;
    int64_t *d_ctg = nullptr, *d_so = nullptr, *d_segs = nullptr, *d_runs = nullptr, *d_hist = nullptr, *d_counts = nullptr;
    uint32_t* d_plane = nullptr;
    if ((rc = pv_get(ctx, "km.ctg", 3 * na + 1, &d_ctg))) return rc;
    if ((rc = pv_get(ctx, "km.seg_off", na + 1, &d_so))) return rc;
    if ((rc = pv_get(ctx, "km.segs", (size_t)seg_capacity + 1, &d_segs))) return rc;
    if ((rc = pv_get(ctx, "km.runs", 3 * (size_t)run_capacity + 1, &d_runs))) return rc;
    if ((rc = pv_get(ctx, "km.hist", (size_t)PV_KMER_HIST, &d_hist))) return rc;
    if ((rc = pv_get(ctx, "km.counts", (size_t)12, &d_counts))) return rc;
    if (pos_counts && (rc = pv_get(ctx, "km.plane", (size_t)N + 1, &d_plane))) return rc;
    // the caller's run records stay as they were where none is written (PV_ERR_CAPACITY)
    if (run_capacity) PV_HIP(hipMemcpyAsync(d_runs, runs, (size_t)run_capacity * 24, hipMemcpyHostToDevice, st));
    if ((rc = pv_kmer_table_build_dev(ctx, s.a, s.a_off, n_asm, k, cap, s.table, s.need, d_counts + 8, st))) return rc;
    if ((rc = pv_kmer_count_reads_dev(ctx, s.table, s.need, s.b, s.b_off, n_reads, (int64_t)s.n_b, st))) return rc;
    if ((rc = pv_kmer_support_dev(ctx, s.table, s.need, s.a_off, n_asm, min_count, segment, d_ctg, d_so, seg_capacity, d_segs,
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
    if ((rc = count_check(table_bytes, bases, n_reads, n_bases, part, n_parts))) return rc;
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
    Staged s;
    if ((rc = km_stage(ctx, A, a_off, n_asm, bases, base_off, n_reads, &s))) return rc;
    if (!s.ok()) counts[1] = s.invalid() ? PV_ERR_INVALID : PV_ERR_LIMIT;
    PV_CHECK(!s.invalid(), PV_ERR_INVALID, "kmer spectrum: offsets must start at 0 and not decrease");
    PV_CHECK(s.ok(), PV_ERR_LIMIT, "kmer spectrum: the assembly or the reads hold 2^31 bytes or more");
    hipStream_t st = ctx->stream;
    const size_t np = (size_t)n_parts;
    const int64_t need = s.need, rneed = reads_bytes(slots);
    uint8_t *d_table = s.table, *d_rtable = nullptr;
    int64_t *d_out = nullptr, *d_counts = nullptr;
    if ((rc = pv_get(ctx, "km.rtable", (size_t)rneed, &d_rtable))) return rc;
    if ((rc = pv_get(ctx, "km.spectrum", (size_t)5 * PV_KMER_HIST, &d_out))) return rc;   // the spectrum, then ro_hist
    if ((rc = pv_get(ctx, "km.fcounts", 4 * np + 8, &d_counts))) return rc;                // {build 4, spectrum 2, 0, 0}, a flush's 4 per part
    if ((rc = pv_zero_async(d_out, (size_t)5 * PV_KMER_HIST * 8, st))) return rc;
    if ((rc = pv_kmer_table_build_dev(ctx, s.a, s.a_off, n_asm, k, cap, d_table, need, d_counts, st))) return rc;
    if ((rc = pv_kmer_reads_table_init_dev(ctx, d_rtable, rneed, slots, cap, st))) return rc;
    for (int p = 0; p < n_parts; p++) {
        if ((rc = pv_kmer_count_reads_all_dev(ctx, d_table, need, d_rtable, rneed, s.b, s.b_off, n_reads, (int64_t)s.n_b, p, n_parts, st)))
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
