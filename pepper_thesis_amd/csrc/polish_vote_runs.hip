// polish_vote_runs.hip — the run vote behind the column vote: the reads of the batch the builder was given + the draft bytes
// -> the labels (and read fractions) of every homopolymer run's chunk rows, by the run length most reads spell.
//
// The rule is in include/pepper_hip.h (pv_polish_vote_runs). It runs behind pv_polish_vote_dev on the same labels / acc
// planes, in place, and rewrites only the rows of decided runs, so everything behind the vote runs on it unchanged.
//
// Six launches, no global atomics:
//   k_runs_find     one lane per draft byte: the maximal stretch the byte lies in, whether it is a candidate and whether a
//                   neighbour makes it adjacent -> cover[i] (the candidate's first byte, or -1), run_n at the first byte,
//                   and the per-block sums of candidates seen / skipped. It also clears row_of and dec_L.
//   k_runs_scatter  one workgroup per chunk: the layout verdict, and row_of[byte] = flat row (chunk_id * step + j) of the
//                   byte's base row. Both chunks that share a row write the same value.
//   k_runs_ops      one lane per read: reference position and read offset at the start of every CIGAR word, and the read's end.
//   k_runs_vote     one workgroup per tile of 256 draft bytes, which owns the runs that start in it: the reads that overlap
//                   the tile are compacted 256 at a time, every (run, read) pair costs two binary searches over the read's
//                   words and a byte scan of at most 63 bytes, histograms in LDS (ds_add); then the decision of every run.
//   k_runs_finish   one block: the sums, the status and the first bad chunk -> d_counts.
//   k_runs_write    one workgroup per chunk, under status PV_OK only: the rows of decided runs.
// The histograms are sums of integers and a run has one owner, so the result does not depend on the launch geometry.
#include "polish_stitch_common.hpp"

using namespace pv_chunks;

namespace {

constexpr int VR_THREADS = 256;          // also the tile width in draft bytes
constexpr int VR_MAX_RUN = 48;
constexpr int VR_MAX_LEN = 63;
constexpr int VR_SLOTS = 88;             // runs that can start in a tile: each takes its bytes and a byte that is not a candidate's, >= 3
constexpr int VR_H = VR_MAX_LEN + 3;     // h[0..63], S, V
constexpr int VR_UNDECIDED = 255;
constexpr int VR_FINISH_THREADS = 512;   // (its six scans keep their waves' sums in registers: at 1024 threads they spill to scratch)

struct RunArgs {
    pv_batch_in in;            // device pointers
    int64_t n_reads, n_bases, n_cigar, n_ref;
    const int64_t* ref_off;
    const uint8_t* ref;
    int min_run;
    int overlap;
    uint8_t* lab;
    float* acc;                // may be null: not written
    // workspace
    int32_t* row_of;           // [n_ref] flat row inside its region of the byte's base row, -1: no chunk holds one
    int32_t* cover;            // [n_ref] first byte of the candidate run (not skipped) the byte lies in, else -1
    uint8_t* run_n;            // [n_ref] at a run's first byte: n
    uint8_t* dec_L;            // [n_ref] at a run's first byte: L, VR_UNDECIDED otherwise
    uint32_t* dec_h;           // [n_ref] at a decided run's first byte: h[L]
    uint32_t* dec_V;           // [n_ref] ... and V
    int64_t* op_rp;            // [n_cigar] reference position at the start of the word
    int64_t* op_qp;            // [n_cigar] read offset at the start of the word
    int64_t* read_end;         // [n_reads] reference position behind the last word
    int32_t* blk_seen;         // [find blocks]
    int32_t* blk_skip;
    int32_t* tile_dec;         // [tiles]
    int32_t* tile_chg;
    int32_t* tile_state;
    int64_t n_find_blocks, n_tiles;
};

__device__ __forceinline__ uint32_t upc(uint32_t c) { return c >= 'a' && c <= 'z' ? c - 32 : c; }
__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; }

// the region whose draft bytes hold byte i: the last g with ref_off[g] <= i, inside 0..n_regions-1
__device__ inline int region_of_byte(const int64_t* ref_off, int n_regions, int64_t i) {
    int lo = 0, hi = n_regions;   // first g in [0, n_regions] with ref_off[g] > i
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ref_off[mid] <= i) lo = mid + 1; else hi = mid;
    }
    const int g = lo - 1;
    return g < 0 ? 0 : g >= n_regions ? n_regions - 1 : g;
}

// the maximal stretch of one letter that byte i of the region's bytes [lo, hi) lies in. ok: the letter is one of ACGT and the
// stretch has at most 48 bytes (either scan gives up after 48 steps, so a longer one is seen as longer).
struct Stretch { int64_t s, e; bool ok; };
__device__ inline Stretch stretch_at(const uint8_t* ref, int64_t lo, int64_t hi, int64_t i) {
    Stretch st;
    st.s = st.e = i;
    const uint32_t b = upc(ref[i]);
    if (acgt_index(b) == 4u) { st.ok = false; return st; }
    while (st.s > lo && i - st.s < VR_MAX_RUN && upc(ref[st.s - 1]) == b) st.s--;
    while (st.e + 1 < hi && st.e - i < VR_MAX_RUN && upc(ref[st.e + 1]) == b) st.e++;
    st.ok = st.e - st.s + 1 <= VR_MAX_RUN;
    return st;
}
__device__ inline bool is_candidate(const Stretch& st, int64_t lo, int64_t hi, int min_run) {
    return st.ok && st.e - st.s + 1 >= min_run && st.s - 1 >= lo && st.e + 1 < hi;
}

__global__ __launch_bounds__(VR_THREADS) void k_runs_find(RunArgs a) {
    __shared__ int32_t lds[VR_THREADS / 64];
    const int64_t i = (int64_t)blockIdx.x * VR_THREADS + threadIdx.x;
    int seen = 0, skip = 0;
    if (i < a.n_ref) {
        const int g = region_of_byte(a.ref_off, a.in.n_regions, i);
        const int64_t lo = clamp64(a.ref_off[g], 0, a.n_ref), hi = clamp64(a.ref_off[g + 1], lo, a.n_ref);
        int32_t cov = -1;
        if (i >= lo && i < hi) {
            const Stretch st = stretch_at(a.ref, lo, hi, i);
            if (is_candidate(st, lo, hi, a.min_run)) {
                // the stretches its flanks lie in end at s-1 and start at e+1: their letters differ from the run's
                const bool adj = is_candidate(stretch_at(a.ref, lo, hi, st.s - 1), lo, hi, a.min_run) ||
                                 is_candidate(stretch_at(a.ref, lo, hi, st.e + 1), lo, hi, a.min_run);
                if (!adj) cov = (int32_t)st.s;
                if (i == st.s) {
                    seen = 1;
                    skip = adj;
                    a.run_n[i] = (uint8_t)(st.e - st.s + 1);
                }
            }
        }
        a.cover[i] = cov;
        a.row_of[i] = -1;
        a.dec_L[i] = VR_UNDECIDED;
    }
    int32_t n_seen, n_skip;
    block_excl_scan<VR_THREADS, int32_t>(seen, lds, &n_seen);
    block_excl_scan<VR_THREADS, int32_t>(skip, lds, &n_skip);
    if (threadIdx.x == 0) { a.blk_seen[blockIdx.x] = n_seen; a.blk_skip[blockIdx.x] = n_skip; }
}

// one block per chunk: the verdict on the layout (as the vote's), and the flat row of every base row into row_of
__global__ __launch_bounds__(ST_THREADS) void k_runs_scatter(StitchArgs a, RunArgs m) {
    __shared__ int32_t lds[ST_THREADS / 64];
    const int64_t k = blockIdx.x;
    const bool ordered = chunk_in_order(a, k);
    int bad_pos = 0;
    if (ordered) {
        const int32_t g = a.region[k];
        const int64_t rs = a.rstart[g], o0 = m.ref_off[g], span = m.ref_off[g + 1] - o0;
        const bool inside = o0 >= 0 && span >= 0 && o0 + span <= m.n_ref;
        const int64_t base = k * a.L, row0 = (int64_t)a.cid[k] * a.step;
        for (int j = threadIdx.x; j < a.L; j += ST_THREADS) {
            const int64_t p = a.pos[base + j];
            if (p < 0 || a.idx[base + j] != 0) continue;
            const int64_t rel = p - rs;
            if (!inside || rel < 0 || rel >= span || row0 + j > INT32_MAX) { bad_pos = 1; continue; }
            m.row_of[o0 + rel] = (int32_t)(row0 + j);
        }
    }
    int32_t npos;
    block_excl_scan<ST_THREADS, int32_t>(bad_pos, lds, &npos);
    if (threadIdx.x == 0) a.chunk_bad[k] = (!ordered || npos) ? BAD_ORDER : BAD_NONE;
}

// one lane per read: where every CIGAR word starts, on the draft and in the read. M / = / X take both, I and S the read, D,
// N and P the draft (the builder's columns), H and anything else nothing.
__global__ __launch_bounds__(VR_THREADS) void k_runs_ops(RunArgs a) {
    const int64_t r = (int64_t)blockIdx.x * VR_THREADS + threadIdx.x;
    if (r >= a.n_reads) return;
    const int64_t c0 = clamp64(a.in.cigar_off[r], 0, a.n_cigar), c1 = clamp64(a.in.cigar_off[r + 1], c0, a.n_cigar);
    int64_t rp = a.in.read_pos[r], qp = 0;
    for (int64_t c = c0; c < c1; c++) {
        const uint32_t w = a.in.cigar[c], op = w & 0xFu;
        const int64_t len = w >> 4;
        a.op_rp[c] = rp;
        a.op_qp[c] = qp;
        if (op == PV_CIGAR_MATCH || op == PV_CIGAR_EQUAL || op == PV_CIGAR_DIFF) { rp += len; qp += len; }
        else if (op == PV_CIGAR_IN || op == PV_CIGAR_SOFT_CLIP) qp += len;
        else if (op == PV_CIGAR_DEL || op == PV_CIGAR_REF_SKIP || op == PV_CIGAR_PAD) rp += len;
    }
    a.read_end[r] = rp;
}

// the read offset of the aligned base of read words [c0, c1) at draft position p, or -1: the word that covers p is the last
// one that starts at or before it (later words start behind its end)
__device__ inline int64_t read_offset_at(const RunArgs& a, int64_t c0, int64_t c1, int64_t p) {
    int64_t lo = c0, hi = c1;   // first word that starts behind p
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a.op_rp[mid] <= p) lo = mid + 1; else hi = mid;
    }
    const int64_t c = lo - 1;
    if (c < c0) return -1;
    const uint32_t w = a.in.cigar[c], op = w & 0xFu;
    if (op != PV_CIGAR_MATCH && op != PV_CIGAR_EQUAL && op != PV_CIGAR_DIFF) return -1;
    const int64_t rp = a.op_rp[c];
    if (p >= rp + (int64_t)(w >> 4)) return -1;
    return a.op_qp[c] + (p - rp);
}

// one (run, read) pair: h points at the run's VR_H counters in LDS. s, n, b: the run's first draft position, length, letter.
__device__ inline void vote_pair(const RunArgs& a, uint32_t* h, int64_t s, int n, uint32_t b, int64_t r) {
    const int64_t e = s + n - 1;
    if (a.in.read_pos[r] > s - 1 || a.read_end[r] <= e + 1) return;
    const int64_t c0 = clamp64(a.in.cigar_off[r], 0, a.n_cigar), c1 = clamp64(a.in.cigar_off[r + 1], c0, a.n_cigar);
    const int64_t q0 = read_offset_at(a, c0, c1, s - 1);
    if (q0 < 0) return;
    const int64_t q1 = read_offset_at(a, c0, c1, e + 1);
    if (q1 <= q0) return;
    const int64_t b0 = clamp64(a.in.base_off[r], 0, a.n_bases), b1 = clamp64(a.in.base_off[r + 1], b0, a.n_bases);
    if (q1 >= b1 - b0) return;   // (a CIGAR longer than its read: the builder refuses such a batch)
    atomicAdd(&h[VR_MAX_LEN + 1], 1u);
    const int64_t len = q1 - q0 - 1;
    if (len > VR_MAX_LEN) return;
    const uint8_t* q = a.in.bases + b0;
    if (upc(q[q0]) == b || upc(q[q1]) == b) return;
    for (int64_t x = q0 + 1; x < q1; x++)
        if (upc(q[x]) != b) return;
    atomicAdd(&h[len], 1u);
    atomicAdd(&h[VR_MAX_LEN + 2], 1u);
}

__global__ __launch_bounds__(VR_THREADS) void k_runs_vote(StitchArgs sa, RunArgs a) {
    __shared__ uint32_t s_h[VR_SLOTS * VR_H];
    __shared__ int32_t s_start[VR_SLOTS];
    __shared__ int32_t s_reads[VR_THREADS];
    __shared__ int32_t lds[VR_THREADS / 64];
    const int tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * VR_THREADS, t1 = min(t0 + VR_THREADS, a.n_ref);
    int n_dec = 0, n_chg = 0, n_state = 0;
    const int G = a.in.n_regions;
    for (int g = region_of_byte(a.ref_off, G, t0); g < G; g++) {
        const int64_t lo = clamp64(a.ref_off[g], 0, a.n_ref), hi = clamp64(a.ref_off[g + 1], lo, a.n_ref);
        if (lo >= t1) break;
        if (hi <= t0) continue;
        const int64_t i = t0 + tid;
        const int isrun = i >= lo && i < hi && i < t1 && a.cover[i] == (int32_t)i;
        int32_t nruns;
        const int32_t slot = block_excl_scan<VR_THREADS, int32_t>(isrun, lds, &nruns);
        if (nruns == 0) continue;
        if (nruns > VR_SLOTS) nruns = VR_SLOTS;   // (cannot be met: see VR_SLOTS)
        if (isrun && slot < VR_SLOTS) s_start[slot] = (int32_t)i;
        for (int x = tid; x < VR_SLOTS * VR_H; x += VR_THREADS) s_h[x] = 0;
        __syncthreads();
        const int64_t rs = sa.rstart[g];
        // the draft positions a run of this tile can ask for
        const int64_t wlo = rs + (max(t0, lo) - lo) - 1, whi = rs + (min(t1, hi) - 1 - lo) + VR_MAX_RUN + 1;
        const int64_t r0 = clamp64(a.in.read_off[g], 0, a.n_reads), r1 = clamp64(a.in.read_off[g + 1], r0, a.n_reads);
        for (int64_t rb = r0; rb < r1; rb += VR_THREADS) {
            const int64_t r = rb + tid;
            const int keep = r < r1 && a.in.read_mapq[r] > 0 && a.in.read_pos[r] <= whi && a.read_end[r] > wlo;
            int32_t nk;
            const int32_t at = block_excl_scan<VR_THREADS, int32_t>(keep, lds, &nk);
            if (keep) s_reads[at] = tid;
            __syncthreads();
            for (int pi = tid; pi < nk * nruns; pi += VR_THREADS) {
                const int sl = pi / nk;
                const int32_t st = s_start[sl];
                vote_pair(a, s_h + sl * VR_H, rs + (st - lo), a.run_n[st], upc(a.ref[st]), rb + s_reads[pi - sl * nk]);
            }
            __syncthreads();   // s_reads is filled again in the next round; the histograms are read below
        }
        if (tid < nruns) {
            const uint32_t* h = s_h + tid * VR_H;
            const uint32_t S = h[VR_MAX_LEN + 1], V = h[VR_MAX_LEN + 2];
            const int32_t st = s_start[tid];
            const int n = a.run_n[st];
            if (V >= 1 && 2 * (uint64_t)V > S) {
                int best = -1;
                uint32_t bh = 0;
                for (int len = 0; len <= VR_MAX_LEN; len++) {
                    const uint32_t v = h[len];
                    if (v == 0 || v < bh) continue;
                    // lengths come in ascending order: among equal ones n, else the closer to n, else the one already held
                    if (v > bh || (best != n && (len == n || abs(len - n) < abs(best - n)))) { best = len; bh = v; }
                }
                a.dec_L[st] = (uint8_t)best;
                a.dec_h[st] = bh;
                a.dec_V[st] = V;
                n_dec++;
                n_chg += best != n;
                if (best > n) {   // the insert rows of the span: the flat rows between the flanks' base rows that are no base rows
                    const int32_t ra = a.row_of[st - 1], rz = a.row_of[st + n];
                    const int64_t have = ra >= 0 && rz >= 0 ? (int64_t)rz - ra - 1 - n : -1;
                    n_state += have < best - n;
                }
            }
        }
        __syncthreads();   // s_start and s_h are the next region's
    }
    int32_t t_dec, t_chg, t_state;
    block_excl_scan<VR_THREADS, int32_t>(n_dec, lds, &t_dec);
    block_excl_scan<VR_THREADS, int32_t>(n_chg, lds, &t_chg);
    block_excl_scan<VR_THREADS, int32_t>(n_state, lds, &t_state);
    if (tid == 0) { a.tile_dec[blockIdx.x] = t_dec; a.tile_chg[blockIdx.x] = t_chg; a.tile_state[blockIdx.x] = t_state; }
}

// one block: the sums, the status and the first bad chunk -> d_counts[6]
__global__ __launch_bounds__(VR_FINISH_THREADS) void k_runs_finish(StitchArgs sa, RunArgs a) {
    __shared__ int64_t lds[VR_FINISH_THREADS / 64];
    __shared__ int64_t s_bad[VR_FINISH_THREADS / 64];
    int64_t seen = 0, skip = 0, dec = 0, chg = 0, state = 0, bad = INT64_MAX;
    for (int64_t k = threadIdx.x; k < a.n_find_blocks; k += VR_FINISH_THREADS) { seen += a.blk_seen[k]; skip += a.blk_skip[k]; }
    for (int64_t k = threadIdx.x; k < a.n_tiles; k += VR_FINISH_THREADS) {
        dec += a.tile_dec[k]; chg += a.tile_chg[k]; state += a.tile_state[k];
    }
    for (int64_t k = threadIdx.x; k < sa.n_chunks; k += VR_FINISH_THREADS)
        if (sa.chunk_bad[k] != BAD_NONE && k < bad) bad = k;
    int64_t n_seen, n_skip, n_dec, n_chg, n_state, nbad;
    block_excl_scan<VR_FINISH_THREADS, int64_t>(seen, lds, &n_seen);
    block_excl_scan<VR_FINISH_THREADS, int64_t>(skip, lds, &n_skip);
    block_excl_scan<VR_FINISH_THREADS, int64_t>(dec, lds, &n_dec);
    block_excl_scan<VR_FINISH_THREADS, int64_t>(chg, lds, &n_chg);
    block_excl_scan<VR_FINISH_THREADS, int64_t>(state, lds, &n_state);
    block_excl_scan<VR_FINISH_THREADS, int64_t>(bad != INT64_MAX ? 1 : 0, lds, &nbad);
    bad = block_first_bad<VR_FINISH_THREADS>(bad, s_bad);
    if (threadIdx.x == 0) {
        const int64_t status = nbad ? PV_ERR_INVALID : n_state ? PV_ERR_STATE : PV_OK;
        sa.counts[0] = status == PV_OK ? n_dec : 0;
        sa.counts[1] = status;
        sa.counts[2] = nbad ? bad : -1;
        sa.counts[3] = status == PV_OK ? n_chg : 0;
        sa.counts[4] = n_seen;
        sa.counts[5] = n_skip;
    }
}

// one block per chunk, under status PV_OK only: the rows of decided runs
__global__ __launch_bounds__(ST_THREADS) void k_runs_write(StitchArgs a, RunArgs m) {
#pragma clang fp contract(off)
    if (a.counts[1] != PV_OK) return;
    const int64_t k = blockIdx.x;
    const int32_t g = a.region[k];
    const int64_t rs = a.rstart[g], o0 = m.ref_off[g], span = m.ref_off[g + 1] - o0;   // (status OK: inside [0, n_ref])
    const int64_t base = k * a.L, row0 = (int64_t)a.cid[k] * a.step;
    for (int j = threadIdx.x; j < a.L; j += ST_THREADS) {
        const int64_t p = a.pos[base + j];
        const int32_t x = a.idx[base + j];
        if (p < 0 || x < 0) continue;
        const int64_t rel = p - rs;
        if (rel < 0 || rel >= span) continue;   // (an insert row's anchor: the layout check looks at base rows)
        const int64_t gi = o0 + rel;
        int64_t st = m.cover[gi];
        if (st < 0) {   // the insert rows in front of a run's first base belong to it too
            if (x > 0 && rel + 1 < span && m.cover[gi + 1] == (int32_t)(gi + 1)) st = gi + 1;
            else continue;
        }
        const int L = m.dec_L[st];
        if (L == VR_UNDECIDED) continue;
        const int n = m.run_n[st];
        const int bl = (int)acgt_index(upc(m.ref[st])) + 1;
        int label;
        if (x == 0) label = (L <= n && gi - st < n - L) ? 0 : bl;
        else if (L <= n) label = 0;
        else {   // the span's insert rows in front of this one: the flat rows behind the left flank's base row but the base rows
            const int64_t rank = row0 + j - m.row_of[st - 1] - 1 - (gi - st + 1);
            label = rank < L - n ? bl : 0;
        }
        m.lab[base + j] = (uint8_t)label;
        if (m.acc) {
            const float wj = (j < m.overlap || j >= a.L - m.overlap) ? 1.0f : 2.0f;
            const float f = wj * ((float)m.dec_h[st] / (float)m.dec_V[st]);
            float* dst = m.acc + (base + j) * 5;
#pragma unroll
            for (int s = 0; s < 5; s++) dst[s] = s == label ? f : 0.0f;
        }
    }
}

// what both forms refuse before they touch the device
int runs_check(int64_t n_chunks, int seq_length, int seq_overlap, int min_run) {
    PV_CHECK(n_chunks >= 0 && seq_length >= 1, PV_ERR_INVALID, "negative sizes");
    PV_CHECK(seq_overlap >= 0 && 2 * (int64_t)seq_overlap <= seq_length, PV_ERR_INVALID,
             "run vote: need 0 <= 2 * seq_overlap <= seq_length (got %d, %d)", seq_length, seq_overlap);
    PV_CHECK(min_run >= 2 && min_run <= VR_MAX_RUN, PV_ERR_INVALID, "run vote: min_run must be in 2..%d (got %d)", VR_MAX_RUN, min_run);
    return PV_OK;
}

}  // namespace

extern "C" int pv_polish_vote_runs_dev(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const pv_batch_in* in,
                                       int64_t n_reads, int64_t n_bases, int64_t n_cigar, int64_t n_ref_bytes,
                                       const int64_t* region_start, const int64_t* ref_off, const uint8_t* ref, int32_t n_regions,
                                       int seq_length, int seq_overlap, int min_run, uint8_t* labels, float* acc,
                                       int64_t* d_counts, void* stream) {
    PV_CHECK(ctx && chunks && in && d_counts, PV_ERR_INVALID, "null argument");
    PV_CHECK(n_regions >= 0 && n_reads >= 0 && n_bases >= 0 && n_cigar >= 0 && n_ref_bytes >= 0, PV_ERR_INVALID, "negative sizes");
    int rc;
    if ((rc = runs_check(n_chunks, seq_length, seq_overlap, min_run))) return rc;
    PV_CHECK(((uintptr_t)acc & 3) == 0, PV_ERR_INVALID, "acc is not aligned to a float");
    PV_CHECK(n_chunks <= chunks->chunk_capacity, PV_ERR_INVALID, "n_chunks %lld exceeds the chunk capacity %lld",
             (long long)n_chunks, (long long)chunks->chunk_capacity);
    PV_CHECK(n_chunks < (1ll << 31), PV_ERR_LIMIT, "too many chunks for one launch");
    PV_CHECK(n_ref_bytes < (1ll << 31) - VR_THREADS && n_reads < (1ll << 31) - VR_THREADS, PV_ERR_LIMIT,
             "too many draft bytes or reads for one launch");
    const bool work = n_chunks > 0 && n_ref_bytes > 0;
    PV_CHECK(n_chunks == 0 || (chunks->position && chunks->index && chunks->region && chunks->chunk_id && labels && region_start &&
                               ref_off && n_regions > 0 && in->n_regions == n_regions),
             PV_ERR_INVALID, "chunk arrays, labels, region starts or draft offsets missing, or the batch holds other regions");
    PV_CHECK(n_chunks == 0 || ref, PV_ERR_INVALID, "run vote: the batch carries no draft bytes (ref is null)");
    PV_CHECK(!work || (in->read_off && (n_reads == 0 || (in->read_pos && in->read_mapq && in->base_off && in->cigar_off)) &&
                       (n_bases == 0 || in->bases) && (n_cigar == 0 || in->cigar)),
             PV_ERR_INVALID, "run vote: read arrays missing");
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = pv_pick_stream(ctx, stream);
    StitchArgs a = chunk_args(chunks, nullptr, region_start, work ? n_chunks : 0, n_regions, seq_length, seq_overlap, d_counts);
    RunArgs m;
    memset(&m, 0, sizeof(m));
    m.in = *in;
    m.n_reads = n_reads; m.n_bases = n_bases; m.n_cigar = n_cigar; m.n_ref = n_ref_bytes;
    m.ref_off = ref_off; m.ref = ref;
    m.min_run = min_run; m.overlap = seq_overlap;
    m.lab = labels; m.acc = acc;
    const int64_t n_tiles = work ? (n_ref_bytes + VR_THREADS - 1) / VR_THREADS : 0;
    m.n_find_blocks = m.n_tiles = n_tiles;
    const size_t nr = (size_t)(n_ref_bytes > 0 ? n_ref_bytes : 1), nc = (size_t)(n_cigar > 0 ? n_cigar : 1);
    const size_t nt = (size_t)(n_tiles > 0 ? n_tiles : 1);
    if ((rc = pv_get(ctx, "runs.bad", (size_t)(n_chunks > 0 ? n_chunks : 1), &a.chunk_bad))) return rc;
    if ((rc = pv_get(ctx, "runs.row_of", nr, &m.row_of))) return rc;
    if ((rc = pv_get(ctx, "runs.cover", nr, &m.cover))) return rc;
    if ((rc = pv_get(ctx, "runs.run_n", nr, &m.run_n))) return rc;
    if ((rc = pv_get(ctx, "runs.dec_L", nr, &m.dec_L))) return rc;
    if ((rc = pv_get(ctx, "runs.dec_h", nr, &m.dec_h))) return rc;
    if ((rc = pv_get(ctx, "runs.dec_V", nr, &m.dec_V))) return rc;
    if ((rc = pv_get(ctx, "runs.op_rp", nc, &m.op_rp))) return rc;
    if ((rc = pv_get(ctx, "runs.op_qp", nc, &m.op_qp))) return rc;
    if ((rc = pv_get(ctx, "runs.read_end", (size_t)(n_reads > 0 ? n_reads : 1), &m.read_end))) return rc;
    if ((rc = pv_get(ctx, "runs.blk_seen", nt, &m.blk_seen))) return rc;
    if ((rc = pv_get(ctx, "runs.blk_skip", nt, &m.blk_skip))) return rc;
    if ((rc = pv_get(ctx, "runs.tile_dec", nt, &m.tile_dec))) return rc;
    if ((rc = pv_get(ctx, "runs.tile_chg", nt, &m.tile_chg))) return rc;
    if ((rc = pv_get(ctx, "runs.tile_state", nt, &m.tile_state))) return rc;
    pv_prof_scope ps_all(ctx, "polish_vote_runs", st);
    if (work) {
        { pv_prof_scope ps(ctx, "k_runs_find", st); k_runs_find<<<(unsigned)n_tiles, VR_THREADS, 0, st>>>(m); }
        { pv_prof_scope ps(ctx, "k_runs_scatter", st); k_runs_scatter<<<(unsigned)n_chunks, ST_THREADS, 0, st>>>(a, m); }
        if (n_reads > 0) {
            pv_prof_scope ps(ctx, "k_runs_ops", st);
            k_runs_ops<<<(unsigned)((n_reads + VR_THREADS - 1) / VR_THREADS), VR_THREADS, 0, st>>>(m);
        }
        { pv_prof_scope ps(ctx, "k_runs_vote", st); k_runs_vote<<<(unsigned)n_tiles, VR_THREADS, 0, st>>>(a, m); }
    }
    k_runs_finish<<<1, VR_FINISH_THREADS, 0, st>>>(a, m);
    if (work) { pv_prof_scope ps(ctx, "k_runs_write", st); k_runs_write<<<(unsigned)n_chunks, ST_THREADS, 0, st>>>(a, m); }
    PV_HIP(hipGetLastError());
    return PV_OK;
}

extern "C" int pv_polish_vote_runs(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const pv_batch_in* in, int seq_length,
                                   int seq_overlap, int min_run, uint8_t* labels, float* acc, int64_t* counts) {
    PV_CHECK(ctx && chunks && in && counts, PV_ERR_INVALID, "null argument");
    int rc;   // everything the call itself refuses is refused here, before a byte is copied to the device
    if ((rc = runs_check(n_chunks, seq_length, seq_overlap, min_run))) return rc;
    PV_CHECK(n_chunks == 0 || labels, PV_ERR_INVALID, "labels missing");
    PV_CHECK(n_chunks == 0 || (in->n_regions > 0 && in->ref), PV_ERR_INVALID, "run vote: the batch carries no regions or no draft bytes");
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    pv_batch_in dev;
    int64_t totals[4];
    if ((rc = pv_upload_batch(ctx, in, &dev, totals, st))) return rc;
    const size_t nc = (size_t)n_chunks, L = (size_t)seq_length;
    pv_polish_out d;
    uint8_t* d_lab = nullptr;
    float* d_acc = nullptr;
    int64_t* d_counts = nullptr;
    if ((rc = stage_chunks(ctx, "vr", chunks, nc, L, false, false, &d, st))) return rc;
    if ((rc = stage(ctx, "vr.labels", (const uint8_t*)labels, nc * L, &d_lab, st))) return rc;
    if (acc && (rc = stage(ctx, "vr.acc", (const float*)acc, nc * L * 5, &d_acc, st))) return rc;
    if ((rc = pv_get(ctx, "vr.counts", (size_t)6, &d_counts))) return rc;
    rc = pv_polish_vote_runs_dev(ctx, &d, n_chunks, &dev, totals[0], totals[1], totals[2], totals[3], dev.ref_start, dev.ref_off,
                                 dev.ref, in->n_regions, seq_length, seq_overlap, min_run, d_lab, acc ? d_acc : nullptr, d_counts, st);
    if (rc) return rc;
    PV_HIP(hipMemcpyAsync(counts, d_counts, 6 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    PV_HIP(hipStreamSynchronize(st));
    const int64_t status = counts[1];
    PV_CHECK(status != PV_ERR_INVALID, PV_ERR_INVALID,
             "run vote: chunk %lld breaks the layout (regions ascending, chunk ids 0,1,2,... inside a region, base positions inside "
             "the region's draft bytes)", (long long)counts[2]);
    PV_CHECK(status != PV_ERR_STATE, PV_ERR_STATE, "run vote: a run's winner needs more insert rows than the chunks hold");
    PV_CHECK(status == PV_OK, (int)status, "run vote: device status %lld", (long long)status);
    if (nc * L > 0) {
        PV_HIP(hipMemcpyAsync(labels, d_lab, nc * L, hipMemcpyDeviceToHost, st));
        if (acc) PV_HIP(hipMemcpyAsync(acc, d_acc, nc * L * 5 * sizeof(float), hipMemcpyDeviceToHost, st));
        PV_HIP(hipStreamSynchronize(st));
    }
    return PV_OK;
}
