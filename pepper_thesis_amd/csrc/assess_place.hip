// assess_place.hip — place assembly contigs on the truth by content: which truth contig, which strand, which interval, from
// 32-mers of the assembly, sampled every `step` bases, that occur exactly once in the truth on either strand.
//
// The rule is in include/pepper_hip.h (pv_assess_place). The truth is the large side, so the search is inverted: the samples'
// keys (x and rc(x), each with its sample and strand) are sorted on the device and the truth streams past that table once.
// The launches, all on one stream, no host read-back:
//   k_pl_setup        one block: the offsets' check, the contigs' sample offsets, what the call needs, its status
//   k_pl_keys         one lane per sample: the key and its reverse complement -> two table entries; their counts and smallest
//                     positions start at 0 and "none"
//   k_pl_sort_local   the bitonic sort of kmer_index.hpp (spans of PL_SORT entries in LDS, the wider steps one launch each),
//   k_pl_sort_global  ordered tried entries first, then by key
//   k_pl_dir          where the keys of each value of the top 12 bits begin in the sorted table
//   k_pl_scan         THE HOT PATH. The tile walk of kmer_index.hpp over the truth, PV_ASSESS_PLACE_TILE bytes and a 31-byte
//                     halo at a time; its visitor finds a position's forward key in the table (the directory, copied to LDS,
//                     leaves a binary search of log2(entries / 4096) steps in L2) and, for every entry with that key, adds
//                     one to the entry's count and keeps the smallest (truth contig, position). Integer atomics: counts and
//                     minima do not depend on the order, nor on how many workgroups share the tiles
//   k_pl_decide       one workgroup per assembly contig: its hits per (truth contig, strand) in LDS, the winner, the interval,
//                     the record
// 5 + the sort's launches: with P the table's capacity (two entries per sample the scratch could hold) rounded up to a power of
// two and m = max(0, log2(P) - 11), the sort takes 1 + m + m (m + 1) / 2 launches (1 for a thousand samples, 21 for thirty
// thousand).
// A status other than PV_OK makes every later kernel return at once, and k_pl_decide poison the records (bytes 0xFF).
#include "kmer_index.hpp"
#include "pv_common.hpp"

namespace {

constexpr int PL_K = PV_ASSESS_K;
constexpr int PL_TILE = PV_ASSESS_PLACE_TILE;   // a lane takes PL_TILE / AS_THREADS consecutive positions
constexpr int PL_SORT = 2048;                   // entries a workgroup sorts in LDS
constexpr int PL_DIR = KI_DIR, PL_SHIFT = 64 - KI_DIR_BITS;   // the directory indexes the top bits of all 64
constexpr int PL_MAX_TRUTH = PV_ASSESS_PLACE_MAX_TRUTH;
constexpr uint64_t PL_NONE = ~0ull;
constexpr uint32_t PL_UNTRIED = 1u << 31;       // in an entry's tag: the sample is not tried; such entries sort behind all others
static_assert(PL_TILE % AS_THREADS == 0 && sizeof(pv_assess_placement) == 40, "tile and record layout");

// the scratch area: offsets in bytes, all multiples of 256. Entry e = 2 * sample + strand.
//   sample_off int64 [n_asm + 1]   the contigs' first samples
//   dir        uint32 [PL_DIR + 1] the sorted table's directory
//   keys       uint64 [2 S]        sorted by (untried, key)
//   tags       uint32 [2 S]        the entry a sorted key belongs to, PL_UNTRIED set for an untried sample's
//   cnt        uint64 [2 S]        by entry: occurrences of its key in the truth; PL_NONE: the sample is not tried
//   pos        uint64 [2 S]        by entry: the smallest (truth contig << 32 | position), PL_NONE without one
struct Layout { int64_t sample_off, dir, keys, tags, cnt, pos, total; };
__host__ __device__ inline Layout pl_layout(int64_t n_asm, int64_t samples) {
    Layout y;
    y.sample_off = 0;
    y.dir = up256((n_asm + 1) * 8);
    y.keys = y.dir + up256((PL_DIR + 1) * 4);
    y.tags = y.keys + up256(samples * 16);
    y.cnt = y.tags + up256(samples * 8);
    y.pos = y.cnt + up256(samples * 16);
    y.total = y.pos + up256(samples * 16);
    return y;
}
__host__ __device__ inline int64_t samples_of(int64_t na, int64_t step) { return na >= PL_K ? (na - PL_K) / step + 1 : 0; }

struct Args {
    const uint8_t* A; const int64_t* a_off;
    const uint8_t* B; const int64_t* b_off;
    int64_t n_asm, n_truth;
    int64_t step;
    int min_hits;
    pv_assess_placement* recs;
    uint8_t* scratch; int64_t scratch_bytes;
    int64_t* counts;   // {records written, status, first bad contig or -1, scratch bytes needed}
};

struct Table { int64_t n; uint32_t* dir; uint64_t* keys; uint32_t* tags; uint64_t* cnt; uint64_t* pos; };
__device__ inline const int64_t* sample_off_of(const Args& g) { return (const int64_t*)g.scratch; }
__device__ inline Table table_of(const Args& g) {
    const int64_t S = sample_off_of(g)[g.n_asm];
    const Layout y = pl_layout(g.n_asm, S);
    return {2 * S, (uint32_t*)(g.scratch + y.dir), (uint64_t*)(g.scratch + y.keys), (uint32_t*)(g.scratch + y.tags),
            (uint64_t*)(g.scratch + y.cnt), (uint64_t*)(g.scratch + y.pos)};
}

// the key of the reverse complement: the complement of a code is its bitwise not, and the 32 codes change places
__device__ inline uint64_t rc_key(uint64_t x) {
    uint64_t y = ~x;
    y = ((y >> 2) & 0x3333333333333333ull) | ((y & 0x3333333333333333ull) << 2);
    y = ((y >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((y & 0x0F0F0F0F0F0F0F0Full) << 4);
    return __builtin_bswap64(y);
}

__global__ __launch_bounds__(AS_THREADS) void k_pl_setup(Args g) {
    __shared__ int64_t lds[AS_THREADS / 64];
    __shared__ unsigned long long s_bad;
    if (threadIdx.x == 0) s_bad = PL_NONE;
    __syncthreads();
    // offsets that decrease, or a contig of 2^31 bytes or more: assembly contig p counts as p, truth contig t as n_asm + t
    for (int64_t p = threadIdx.x; p < g.n_asm + g.n_truth; p += AS_THREADS) {
        const int64_t* off = p < g.n_asm ? g.a_off + p : g.b_off + (p - g.n_asm);
        const int64_t n = off[1] - off[0];
        if (n < 0 || n >= (1ll << 31)) atomicMin(&s_bad, (unsigned long long)p);
    }
    __syncthreads();
    const unsigned long long bad = s_bad;
    const int64_t step = g.step;
    const int64_t S = block_scan_to(g.n_asm, (int64_t*)g.scratch, lds, [&](int64_t p) {
        return bad != PL_NONE ? (int64_t)0 : samples_of(g.a_off[p + 1] - g.a_off[p], step);
    });
    if (threadIdx.x == 0) {
        const Layout y = pl_layout(g.n_asm, S);
        const int64_t status = bad != PL_NONE ? PV_ERR_INVALID : (S >= (1ll << 30) || y.total > g.scratch_bytes) ? PV_ERR_LIMIT : PV_OK;
        g.counts[0] = status == PV_OK ? g.n_asm : 0;
        g.counts[1] = status;
        g.counts[2] = bad != PL_NONE ? (int64_t)bad : -1;
        g.counts[3] = y.total;
    }
}

__global__ __launch_bounds__(AS_THREADS) void k_pl_keys(Args g) {
    if (g.counts[1] != PV_OK) return;
    const int64_t* sample_off = sample_off_of(g);
    const Table tb = table_of(g);
    const int64_t S = tb.n / 2;
    for (int64_t s = (int64_t)blockIdx.x * AS_THREADS + threadIdx.x; s < S; s += (int64_t)gridDim.x * AS_THREADS) {
        const int64_t p = owner_of(sample_off, g.n_asm, s);
        const uint8_t* kmer = g.A + g.a_off[p] + (s - sample_off[p]) * g.step;
        uint64_t x = 0;
        bool acgt = true;
        for (int q = 0; q < PL_K; q++) {
            const uint32_t c = code_of(kmer[q]);
            acgt = acgt && c < 4;
            x = (x << 2) | (c & 3);
        }
        const uint64_t r = rc_key(x);
        const bool tried = acgt && x != r;   // a palindrome cannot tell the strand
        const uint32_t e = (uint32_t)(2 * s), flag = tried ? 0 : PL_UNTRIED;
        tb.keys[e] = tried ? x : PL_NONE;
        tb.keys[e + 1] = tried ? r : PL_NONE;
        tb.tags[e] = e | flag;
        tb.tags[e + 1] = (e + 1) | flag;
        tb.cnt[e] = tb.cnt[e + 1] = tried ? 0 : PL_NONE;
        tb.pos[e] = tb.pos[e + 1] = PL_NONE;
    }
}

// ---- the sort ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AS_THREADS) void k_pl_sort_local(Args g, int tail) {
    if (g.counts[1] != PV_OK) return;
    const Table tb = table_of(g);
    sort_spans<PL_SORT, TriedThenKey>(tb.keys, tb.tags, tb.n, tail);
}

__global__ __launch_bounds__(AS_THREADS) void k_pl_sort_global(Args g, int64_t j, int mirror) {
    if (g.counts[1] != PV_OK) return;
    const Table tb = table_of(g);
    sort_global_step<TriedThenKey>(tb.keys, tb.tags, tb.n, j, mirror);
}

__global__ __launch_bounds__(AS_THREADS) void k_pl_dir(Args g) {
    if (g.counts[1] != PV_OK) return;
    const Table tb = table_of(g);
    const int b = blockIdx.x * AS_THREADS + threadIdx.x;
    if (b < PL_DIR) tb.dir[b] = dir_entry(tb.keys, tb.n, b, PL_SHIFT);
    else if (b == PL_DIR) tb.dir[b] = (uint32_t)tb.n;   // (PL_DIR << PL_SHIFT is 2^64)
}

// ---- the pass over the truth -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AS_THREADS) void k_pl_scan(Args g) {
    __shared__ uint8_t s_code[PL_TILE + PL_K];
    __shared__ uint32_t s_dir[PL_DIR + 1];
    if (g.counts[1] != PV_OK) return;
    const int64_t lo = g.b_off[0], hi = g.b_off[g.n_truth];
    if (lo + (int64_t)blockIdx.x * PL_TILE >= hi) return;
    const Table tb = table_of(g);
    if (tb.n == 0) return;
    for (int b = threadIdx.x; b <= PL_DIR; b += AS_THREADS) s_dir[b] = tb.dir[b];
    // a 32-mer lies inside one truth contig; only its forward key is looked up: the table holds both strands of a sample
    tile_walk<PL_TILE>(g.B, g.b_off, g.n_truth, lo, hi, PL_K, s_code, [] {}, [&](const Roll& r, int64_t pos, int64_t t, int64_t start) {
        const uint64_t key = r.fwd, packed = ((uint64_t)t << 32) | (uint64_t)(pos - start);
        // equal keys: the same 32-mer sampled more than once
        for (int64_t e = dir_find(s_dir, tb.keys, key, PL_SHIFT).e; e < tb.n && tb.keys[e] == key; e++) {
            const uint32_t tag = tb.tags[e];
            if (tag & PL_UNTRIED) break;   // (the untried entries' key is a real one, T x 32, and they follow the tried)
            atomicAdd((unsigned long long*)&tb.cnt[tag], 1ull);
            atomicMin((unsigned long long*)&tb.pos[tag], (unsigned long long)packed);
        }
    });
}

// ---- the decision -----------------------------------------------------------------------------------------------------------
// a hit of sample s (entry pair e, e + 1), if it is one: strand and packed (truth contig, position)
__device__ inline bool hit_of(const Table& tb, int64_t s, int* strand, uint64_t* packed) {
    const uint64_t f = tb.cnt[2 * s], r = tb.cnt[2 * s + 1];
    if (f == PL_NONE || f + r != 1) return false;
    *strand = r == 1;
    *packed = tb.pos[2 * s + *strand];
    return true;
}

__global__ __launch_bounds__(AS_THREADS) void k_pl_decide(Args g) {
    extern __shared__ uint32_t s_tally[];   // [2 n_truth]: hits of (t, strand) at 2 t + strand
    __shared__ uint64_t s_red[AS_THREADS / 64];
    const int64_t p = blockIdx.x;
    if (g.counts[1] != PV_OK) {
        if (threadIdx.x < sizeof(pv_assess_placement) / 8) ((int64_t*)(g.recs + p))[threadIdx.x] = -1;
        return;
    }
    const int64_t* sample_off = sample_off_of(g);
    const Table tb = table_of(g);
    const int64_t s0 = sample_off[p], ns = sample_off[p + 1] - s0;
    const int64_t na = g.a_off[p + 1] - g.a_off[p];
    for (int i = threadIdx.x; i < 2 * g.n_truth; i += AS_THREADS) s_tally[i] = 0;
    __syncthreads();
    uint64_t tried = 0, hits = 0;
    for (int64_t s = threadIdx.x; s < ns; s += AS_THREADS) {
        tried += tb.cnt[2 * (s0 + s)] != PL_NONE;
        int strand;
        uint64_t packed;
        if (hit_of(tb, s0 + s, &strand, &packed)) {
            hits++;
            atomicAdd(&s_tally[2 * (packed >> 32) + strand], 1u);
        }
    }
    __syncthreads();
    const auto most = [](uint64_t a, uint64_t b) { return a > b ? a : b; };
    const auto least = [](uint64_t a, uint64_t b) { return a < b ? a : b; };
    tried = block_reduce(tried, s_red, as_add());
    hits = block_reduce(hits, s_red, as_add());
    // the winner: the most hits, ties to the smaller 2 t + strand (the smaller t, then the forward strand)
    uint64_t best = 0;
    for (uint32_t i = threadIdx.x; i < 2 * g.n_truth; i += AS_THREADS) best = most(best, ((uint64_t)s_tally[i] << 32) | (0xFFFFFFFFu - i));
    best = block_reduce(best, s_red, most);
    const int64_t H = (int64_t)(best >> 32), N = (int64_t)hits;
    const uint32_t win = 0xFFFFFFFFu - (uint32_t)best;
    const bool placed = H >= g.min_hits && 2 * H > N;
    // the winner's hits with the smallest and the largest position in the oriented contig: (a' << 32 | j), a' < 2^31
    uint64_t first = PL_NONE, last = 0;
    if (placed) {
        for (int64_t s = threadIdx.x; s < ns; s += AS_THREADS) {
            int strand;
            uint64_t packed;
            if (!hit_of(tb, s0 + s, &strand, &packed) || 2 * (packed >> 32) + strand != win) continue;
            const int64_t a = s * g.step, ao = strand ? na - PL_K - a : a;
            const uint64_t v = ((uint64_t)ao << 32) | (uint32_t)packed;
            first = least(first, v);
            last = most(last, v);
        }
        first = block_reduce(first, s_red, least);
        last = block_reduce(last, s_red, most);
    }
    if (threadIdx.x != 0) return;
    pv_assess_placement o;
    o.b_lo = o.b_hi = -1; o.truth = o.strand = -1;
    o.status = PV_ASSESS_UNPLACED;
    o.tried = (int32_t)tried; o.hits = (int32_t)N; o.agree = (int32_t)H;
    if (placed) {
        const int64_t t = win >> 1, nb = g.b_off[t + 1] - g.b_off[t];
        const int64_t a_first = (int64_t)(first >> 32), j_first = (int64_t)(uint32_t)first;
        const int64_t a_last = (int64_t)(last >> 32), j_last = (int64_t)(uint32_t)last;
        o.truth = (int32_t)t; o.strand = (int32_t)(win & 1);
        o.b_lo = min(max(j_first - a_first, (int64_t)0), nb);
        o.b_hi = min(max(j_last + (na - a_last), (int64_t)0), nb);
        // the hits agree on a contig and a strand but not on an order
        o.status = (first != last && j_last <= j_first) || o.b_hi <= o.b_lo ? PV_ASSESS_MISPLACED : PV_ASSESS_PLACED;
    }
    g.recs[p] = o;
}

// the status is known to the host alone (nothing to place, too many truth contigs, a scratch that cannot hold even the sample
// offsets): the counts, and under a status other than PV_OK poison in every record
__global__ __launch_bounds__(AS_THREADS) void k_pl_finish(Args g, int64_t status, int64_t need) {
    const int64_t t = (int64_t)blockIdx.x * AS_THREADS + threadIdx.x;
    if (status != PV_OK && t < g.n_asm * (int64_t)(sizeof(pv_assess_placement) / 8)) ((int64_t*)g.recs)[t] = -1;
    if (t == 0) { g.counts[0] = 0; g.counts[1] = status; g.counts[2] = -1; g.counts[3] = need; }
}

int place_check(int64_t n_asm, int64_t n_truth, int step, int min_hits) {
    PV_CHECK(n_asm >= 0 && n_truth >= 0, PV_ERR_INVALID, "assess place: negative sizes");
    PV_CHECK(n_asm < (1ll << 31), PV_ERR_LIMIT, "assess place: too many contigs for one launch");
    PV_CHECK(step >= 32 && step <= 65536 && step % 32 == 0, PV_ERR_INVALID,
             "assess place: step must be a multiple of 32 in [32, 65536] (got %d)", step);
    PV_CHECK(min_hits >= 1 && min_hits <= 65535, PV_ERR_INVALID, "assess place: min_hits must lie in [1, 65535] (got %d)", min_hits);
    return PV_OK;
}

}  // namespace

extern "C" int64_t pv_assess_place_scratch_bytes(int64_t n_asm, const int64_t* a_off, int step) {
    if (n_asm < 0 || (n_asm > 0 && !a_off) || step < 1) return PV_ERR_INVALID;
    int64_t samples = 0;
    for (int64_t p = 0; p < n_asm; p++) {
        const int64_t na = a_off[p + 1] - a_off[p];
        if (na < 0) return PV_ERR_INVALID;
        samples += samples_of(na, step);
    }
    return pl_layout(n_asm, samples).total;
}

extern "C" int pv_assess_place_dev(pv_ctx* ctx, const uint8_t* A, const int64_t* a_off, int64_t n_asm, const uint8_t* B,
                                   const int64_t* b_off, int64_t n_truth, int step, int min_hits, pv_assess_placement* recs,
                                   void* scratch, int64_t scratch_bytes, int64_t* d_counts, void* stream) {
    PV_CHECK(ctx && d_counts, PV_ERR_INVALID, "assess place: null argument");
    PV_CHECK(scratch_bytes >= 0, PV_ERR_INVALID, "assess place: negative sizes");
    int rc;
    if ((rc = place_check(n_asm, n_truth, step, min_hits))) return rc;
    PV_CHECK(n_asm == 0 || (A && a_off && b_off && recs), PV_ERR_INVALID, "assess place: sequences, offsets or records missing");
    PV_CHECK(n_asm == 0 || n_truth == 0 || B, PV_ERR_INVALID, "assess place: the truth is missing");
    PV_CHECK(scratch_bytes == 0 || scratch, PV_ERR_INVALID, "assess place: scratch missing");
    PV_CHECK(((uintptr_t)scratch & 255) == 0 && ((uintptr_t)recs & 7) == 0, PV_ERR_INVALID,
             "assess place: scratch must be aligned to 256 bytes and the records to 8");
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = pv_pick_stream(ctx, stream);
    pv_prof_scope ps_all(ctx, "assess_place", st);
    Args g = {A, a_off, B, b_off, n_asm, n_truth, step, min_hits, recs, (uint8_t*)scratch, scratch_bytes, d_counts};
    const int64_t head = pl_layout(n_asm, 0).total;   // the least any call with n_asm contigs needs
    const unsigned rec_blocks = blocks_for(n_asm * (int64_t)(sizeof(pv_assess_placement) / 8), AS_THREADS, 1ll << 31);
    if (n_asm == 0) {   // nothing is looked at
        k_pl_finish<<<1, AS_THREADS, 0, st>>>(g, PV_OK, 0);
        PV_HIP(hipGetLastError());
        return PV_OK;
    }
    if (n_truth > PL_MAX_TRUTH || scratch_bytes < head) {
        k_pl_finish<<<rec_blocks, AS_THREADS, 0, st>>>(g, PV_ERR_LIMIT, head);
        PV_HIP(hipGetLastError());
        if (n_truth > PL_MAX_TRUTH)
            pv_set_error("assess place: %lld truth contigs, at most %d", (long long)n_truth, PL_MAX_TRUTH);
        else
            pv_set_error("assess place: the scratch of %lld bytes cannot hold %lld contigs", (long long)scratch_bytes, (long long)n_asm);
        return PV_ERR_LIMIT;
    }
    static uint64_t tally_allowed = 0;   // per device, once: the tally of PL_MAX_TRUTH truth contigs is all of 64 KB
    if (!(tally_allowed >> (ctx->device & 63) & 1)) {
        PV_HIP(hipFuncSetAttribute((const void*)k_pl_decide, hipFuncAttributeMaxDynamicSharedMemorySize, PL_MAX_TRUTH * 8));
        tally_allowed |= 1ull << (ctx->device & 63);
    }
    // what the scratch could hold bounds every grid and the sort's depth; the kernels take the true sizes from the device
    const int64_t entries = std::max<int64_t>(2, 2 * ((scratch_bytes - head) / 56));
    const int64_t wide = 8ll * ctx->num_cu;
    k_pl_setup<<<1, AS_THREADS, 0, st>>>(g);
    k_pl_keys<<<blocks_for(entries / 2, AS_THREADS, wide), AS_THREADS, 0, st>>>(g);
    {
        pv_prof_scope ps(ctx, "k_pl_sort", st);
        const unsigned spans = blocks_for(entries, PL_SORT, wide), pairs = blocks_for(entries / 2, AS_THREADS, wide);
        sort_schedule(entries, PL_SORT, [&](int tail) { k_pl_sort_local<<<spans, AS_THREADS, 0, st>>>(g, tail); },
                      [&](int64_t j, int mirror) { k_pl_sort_global<<<pairs, AS_THREADS, 0, st>>>(g, j, mirror); });
    }
    k_pl_dir<<<PL_DIR / AS_THREADS + 1, AS_THREADS, 0, st>>>(g);
    { pv_prof_scope ps(ctx, "k_pl_scan", st); k_pl_scan<<<(unsigned)(4 * ctx->num_cu), AS_THREADS, 0, st>>>(g); }
    k_pl_decide<<<(unsigned)n_asm, AS_THREADS, (size_t)n_truth * 8, st>>>(g);
    PV_HIP(hipGetLastError());
    return PV_OK;
}

extern "C" int pv_assess_place(pv_ctx* ctx, const uint8_t* A, const int64_t* a_off, int64_t n_asm, const uint8_t* B,
                               const int64_t* b_off, int64_t n_truth, int step, int min_hits, pv_assess_placement* recs,
                               int64_t* counts) {
    PV_CHECK(ctx && counts, PV_ERR_INVALID, "assess place: null argument");
    int rc;
    if ((rc = place_check(n_asm, n_truth, step, min_hits))) return rc;
    PV_CHECK(n_asm == 0 || (A && a_off && b_off && recs), PV_ERR_INVALID, "assess place: sequences, offsets or records missing");
    PV_CHECK(n_asm == 0 || n_truth == 0 || B, PV_ERR_INVALID, "assess place: the truth is missing");
    counts[0] = 0; counts[1] = PV_OK; counts[2] = -1; counts[3] = 0;
    if (n_asm == 0) return PV_OK;
    // the offsets size the copies, so they are looked at here first: what the device would report, reported the same way
    for (int64_t p = 0; p < n_asm + n_truth && counts[2] < 0; p++) {
        const int64_t* off = p < n_asm ? a_off + p : b_off + (p - n_asm);
        if (off[1] < off[0] || off[1] - off[0] >= (1ll << 31)) counts[2] = p;
    }
    if (counts[2] >= 0 || a_off[0] != 0 || b_off[0] != 0) {
        memset(recs, 0xFF, (size_t)n_asm * sizeof(pv_assess_placement));
        counts[1] = PV_ERR_INVALID;
        PV_CHECK(counts[2] < 0, PV_ERR_INVALID, "assess place: the offsets of contig %lld decrease, or it holds 2^31 bytes or more",
                 (long long)counts[2]);
        PV_CHECK(false, PV_ERR_INVALID, "assess place: offsets must start at 0");
    }
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t na = (size_t)n_asm, nt = (size_t)n_truth;
    const size_t n_a = (size_t)a_off[n_asm], n_b = (size_t)b_off[n_truth];
    const int64_t need = pv_assess_place_scratch_bytes(n_asm, a_off, step);
    uint8_t *d_a = nullptr, *d_b = nullptr, *d_scratch = nullptr;
    int64_t *d_ao = nullptr, *d_bo = nullptr, *d_counts = nullptr;
    pv_assess_placement* d_recs = nullptr;
    if ((rc = pv_get(ctx, "pl.a", n_a > 0 ? n_a : 1, &d_a))) return rc;
    if ((rc = pv_get(ctx, "pl.b", n_b > 0 ? n_b : 1, &d_b))) return rc;
    if ((rc = pv_get(ctx, "pl.a_off", na + 1, &d_ao))) return rc;
    if ((rc = pv_get(ctx, "pl.b_off", nt + 1, &d_bo))) return rc;
    if ((rc = pv_get(ctx, "pl.recs", na, &d_recs))) return rc;
    if ((rc = pv_get(ctx, "pl.scratch", (size_t)need, &d_scratch))) return rc;
    if ((rc = pv_get(ctx, "pl.counts", (size_t)4, &d_counts))) return rc;
    if (n_a) PV_HIP(hipMemcpyAsync(d_a, A, n_a, hipMemcpyHostToDevice, st));
    if (n_b) PV_HIP(hipMemcpyAsync(d_b, B, n_b, hipMemcpyHostToDevice, st));
    PV_HIP(hipMemcpyAsync(d_ao, a_off, (na + 1) * 8, hipMemcpyHostToDevice, st));
    PV_HIP(hipMemcpyAsync(d_bo, b_off, (nt + 1) * 8, hipMemcpyHostToDevice, st));
    rc = pv_assess_place_dev(ctx, d_a, d_ao, n_asm, d_b, d_bo, n_truth, step, min_hits, d_recs, d_scratch, need, d_counts, st);
    // under PV_ERR_LIMIT the device form has poisoned the records and set the counts: they come back all the same
    if (rc && rc != PV_ERR_LIMIT) return rc;
    PV_HIP(hipMemcpyAsync(counts, d_counts, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    PV_HIP(hipMemcpyAsync(recs, d_recs, na * sizeof(pv_assess_placement), hipMemcpyDeviceToHost, st));
    PV_HIP(hipStreamSynchronize(st));
    if (rc) return rc;
    PV_CHECK(counts[1] == PV_OK, (int)counts[1], "assess place: device status %lld (%lld bytes of scratch needed)",
             (long long)counts[1], (long long)counts[3]);
    return PV_OK;
}
