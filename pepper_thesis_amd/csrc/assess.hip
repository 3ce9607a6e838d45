// assess.hip — score an assembly against a truth sequence: per contig pair, unique 32-mer anchors every `segment` bases, a
// colinear chain of them, and between consecutive anchors a global alignment in a band of 128 cells whose traceback is
// classified into matches, substitutions, insertions and deletions.
//
// The rule is in include/pepper_hip.h (pv_assess). Seven launches on one stream, no global atomics, no host read-back:
//   k_as_setup    one block: the pairs' slot offsets (floor(n_A / L) + 1 slots each), what the call needs, its status
//   k_as_anchor   one workgroup per slot: the lanes spread over the window's start positions, byte compare with early exit
//   k_as_chain    one workgroup per pair: the anchors staged through LDS, one lane applies the keep rule and writes the segments
//   k_as_offsets  one block: the pairs' segment counts -> pair_seg_off
//   k_as_sweep    one wavefront per segment, two band cells per lane; the left recurrence of a row is the wave's prefix
//                 minimum of T[c] + (128 - c), by shuffles. A lane's two cells give four direction bits per row; eight rows
//                 fill the lane's dword, which the wave stores as 256 contiguous bytes: 32 bytes per row, ordinary vector
//                 stores, nothing crosses lanes to be packed
//   k_as_trace    one lane per segment: walks the direction words back from (n, m) and writes the segment's record
//   k_as_reduce   one workgroup per pair: the records -> the contig's totals
// A status other than PV_OK makes every later kernel poison its outputs instead (bytes 0xFF: every field -1).
//
// pv_assess_errors_dev keeps the traceback's path (the rule: pv_assess_errors in the header). The same seven launches, then:
//   k_as_errcnt   one lane per slot: the aligned segment's sub + ins + del, from its record
//   k_as_erroff   one block: the scan over all slots -> each segment's first error record, pair_err_off, the need, the status
//   k_as_hist     one workgroup per slot: the qualities of the segment's rows and anchor bytes into an LDS table -> the slot's
//                 partial table in the scratch (only with Q)
//   k_as_errors   one lane per slot: the walk of k_as_trace again (as_walk, one template for both), each record stored from the
//                 end of the segment's range; with Q the lane adds its errors to its own slot's partial table
//   k_as_qreduce  one workgroup per pair: the partial tables of its segments, summed in a fixed order -> qhist (only with Q)
//   k_as_epoison  under PV_ERR_INVALID / PV_ERR_LIMIT: 0xFF over errs, pair_err_off and qhist
#include <algorithm>

#include "assess_scan.hpp"
#include "pv_common.hpp"

namespace {

constexpr int AS_K = PV_ASSESS_K, AS_W = PV_ASSESS_W, AS_DMAX = PV_ASSESS_MAX_DIFF;
constexpr uint32_t AS_INF = 0xF0000000u;   // above every distance (< 2^31 + 128); + 129 still fits
enum { DIR_DIAG = 0, DIR_UP = 1, DIR_LEFT = 2 };

struct SegSlot { int64_t a0, b0, n, m; };   // a pair's segments, in its slots of the scratch
struct Anchor { int64_t a, b; };            // a < 0: slot without an anchor

// the scratch area: offsets in bytes, all multiples of 256
struct Layout { int64_t slot_off, pair_cnt, anchors, segs, dirs, err_cnt, err_off, qpart, total; };
constexpr int AS_QTAB = PV_ASSESS_QBINS * 4;   // a slot's partial table: uint32 {bases, sub, ins, del} per quality
// with_err: the per-slot error counts and offsets and the partial quality tables of pv_assess_errors_dev, behind the rest
__host__ __device__ inline Layout as_layout(int64_t n_pairs, int64_t slots, int64_t total_a, int with_err) {
    Layout y;
    y.slot_off = 0;
    y.pair_cnt = up256((n_pairs + 1) * 8);
    y.anchors = y.pair_cnt + up256(n_pairs * 16);
    y.segs = y.anchors + up256(slots * 16);
    y.dirs = y.segs + up256(slots * 32);
    y.err_cnt = y.dirs + up256(32 * total_a + 256 * slots);
    y.err_off = y.err_cnt + (with_err ? up256(slots * 8) : 0);
    y.qpart = y.err_off + (with_err ? up256((slots + 1) * 8) : 0);
    y.total = y.qpart + (with_err ? up256(slots * AS_QTAB * 4) : 0);
    return y;
}

struct Args {
    const uint8_t* A; const int64_t* a_off;
    const uint8_t* B; const int64_t* b_off;
    int64_t n_pairs;
    int64_t L, max_shift;
    int64_t seg_capacity;
    pv_assess_seg* segs;
    int64_t* pair_seg_off;
    int64_t* totals;
    uint8_t* scratch; int64_t scratch_bytes;
    int64_t* counts;   // {segments, status, slots needed, scratch bytes needed}; with_err: int64[8], see ErrArgs
    int with_err;
};
// what pv_assess_errors_dev adds; counts[4..7] = {error records written, needed, 0, 0}
struct ErrArgs {
    const uint8_t* Q;
    int64_t err_capacity;
    pv_assess_error* errs;
    int64_t* pair_err_off;
    int64_t* qhist;
};

__device__ inline int64_t* slot_off_of(const Args& g) { return (int64_t*)g.scratch; }
__device__ inline Layout layout_of(const Args& g) {
    return as_layout(g.n_pairs, slot_off_of(g)[g.n_pairs], g.a_off[g.n_pairs] - g.a_off[0], g.with_err);
}

__global__ __launch_bounds__(AS_THREADS) void k_as_setup(Args g) {
    __shared__ int64_t lds[AS_THREADS / 64];
    __shared__ int s_bad;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    int bad = 0;   // offsets that decrease, or a contig of 2^31 bytes or more
    for (int64_t p = threadIdx.x; p < g.n_pairs; p += AS_THREADS) {
        const int64_t na = g.a_off[p + 1] - g.a_off[p], nb = g.b_off[p + 1] - g.b_off[p];
        if (na < 0 || nb < 0 || na >= (1ll << 31) || nb >= (1ll << 31)) bad = 1;
    }
    if (bad) s_bad = 1;
    __syncthreads();
    bad = s_bad;
    const int64_t L = g.L;
    const int64_t slots = block_scan_to(g.n_pairs, slot_off_of(g), lds, [&](int64_t p) {
        const int64_t na = g.a_off[p + 1] - g.a_off[p];
        return bad ? (int64_t)1 : na / L + 1;
    });
    if (threadIdx.x == 0) {
        const Layout y = as_layout(g.n_pairs, slots, bad ? 0 : g.a_off[g.n_pairs] - g.a_off[0], g.with_err);
        g.counts[0] = 0;
        g.counts[1] = bad ? PV_ERR_INVALID : (slots > g.seg_capacity || y.total > g.scratch_bytes) ? PV_ERR_LIMIT : PV_OK;
        g.counts[2] = slots;
        g.counts[3] = y.total;
        if (g.with_err) { g.counts[4] = 0; g.counts[5] = -1; g.counts[6] = 0; g.counts[7] = 0; }
    }
}

// one workgroup per slot. Slot s of a pair is anchor k = s + 1; the pair's last slot has none.
__global__ __launch_bounds__(AS_THREADS) void k_as_anchor(Args g) {
    __shared__ uint8_t s_kmer[AS_K];
    __shared__ int s_cnt[AS_THREADS / 64];
    __shared__ int64_t s_hit[AS_THREADS / 64];
    if (g.counts[1] != PV_OK) return;
    const int64_t* slot_off = slot_off_of(g);
    const int64_t slot = blockIdx.x;
    if (slot >= slot_off[g.n_pairs]) return;
    const Layout y = layout_of(g);
    Anchor* anchors = (Anchor*)(g.scratch + y.anchors);
    const int64_t p = owner_of(slot_off, g.n_pairs, slot);
    const int64_t k = slot - slot_off[p] + 1;
    const int64_t na = g.a_off[p + 1] - g.a_off[p], nb = g.b_off[p + 1] - g.b_off[p];
    const uint8_t* A = g.A + g.a_off[p];
    const uint8_t* B = g.B + g.b_off[p];
    Anchor found = {-1, -1};
    if (k <= na / g.L) {
        for (int t = 0; t < 8; t++) {   // (everything that steers this loop is the same in every thread)
            const int64_t a = k * g.L + 32 * t;
            if (a + AS_K > na) break;
            __syncthreads();   // the previous candidate's s_kmer, s_cnt and s_hit have been read
            if (threadIdx.x < AS_K) s_kmer[threadIdx.x] = A[a + threadIdx.x];
            __syncthreads();
            bool acgt = true;
            for (int q = 0; q < AS_K; q++) {
                const uint8_t x = s_kmer[q];
                acgt = acgt && (x == 'A' || x == 'C' || x == 'G' || x == 'T');
            }
            if (!acgt) continue;
            const int64_t c = a * nb / na;   // a < 2^31 and nb < 2^31: no overflow
            const int64_t lo = max((int64_t)0, c - g.max_shift), hi = min(nb - AS_K, c + g.max_shift);
            int cnt = 0;
            int64_t hit = -1;
            for (int64_t j = lo + threadIdx.x; j <= hi; j += AS_THREADS) {
                int q = 0;
                while (q < AS_K && B[j + q] == s_kmer[q]) q++;
                if (q == AS_K) { cnt++; hit = j; }
            }
            cnt = wave_sum(cnt);
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) hit = max(hit, __shfl_xor(hit, d, 64));
            if ((threadIdx.x & 63) == 0) { s_cnt[threadIdx.x >> 6] = cnt; s_hit[threadIdx.x >> 6] = hit; }
            __syncthreads();
            cnt = 0; hit = -1;
            for (int i = 0; i < AS_THREADS / 64; i++) { cnt += s_cnt[i]; hit = max(hit, s_hit[i]); }
            if (cnt == 1) { found.a = a; found.b = hit; break; }
        }
    }
    if (threadIdx.x == 0) anchors[slot] = found;
}

// one workgroup per pair: the keep rule, the pair's segments into its slots, their number into pair_cnt
constexpr int CH_STAGE = 1024;
__global__ __launch_bounds__(AS_THREADS) void k_as_chain(Args g) {
    __shared__ Anchor s_anc[CH_STAGE];
    if (g.counts[1] != PV_OK) return;
    const int64_t* slot_off = slot_off_of(g);
    const Layout y = layout_of(g);
    const Anchor* anchors = (const Anchor*)(g.scratch + y.anchors);
    SegSlot* segs = (SegSlot*)(g.scratch + y.segs);
    int64_t* pair_cnt = (int64_t*)(g.scratch + y.pair_cnt);   // [n_pairs][2]: segments, anchors found
    const int64_t p = blockIdx.x;
    const int64_t s0 = slot_off[p], ns = slot_off[p + 1] - s0 - 1;   // anchor slots
    const int64_t na = g.a_off[p + 1] - g.a_off[p], nb = g.b_off[p + 1] - g.b_off[p];
    int64_t ap = -AS_K, bp = -AS_K, n_seg = 0, n_found = 0;   // thread 0's
    for (int64_t base = 0; base < ns; base += CH_STAGE) {
        const int cnt = (int)min((int64_t)CH_STAGE, ns - base);
        __syncthreads();
        for (int i = threadIdx.x; i < cnt; i += AS_THREADS) s_anc[i] = anchors[s0 + base + i];
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int i = 0; i < cnt; i++) {
                const Anchor x = s_anc[i];
                if (x.a < 0) continue;
                n_found++;
                if (x.a >= ap + AS_K && x.b >= bp + AS_K) {
                    segs[s0 + n_seg] = {ap + AS_K, bp + AS_K, x.a - (ap + AS_K), x.b - (bp + AS_K)};
                    n_seg++;
                    ap = x.a; bp = x.b;
                }
            }
        }
    }
    if (threadIdx.x == 0) {
        segs[s0 + n_seg] = {ap + AS_K, bp + AS_K, na - (ap + AS_K), nb - (bp + AS_K)};
        pair_cnt[2 * p] = n_seg + 1;
        pair_cnt[2 * p + 1] = n_found;
    }
}

__global__ __launch_bounds__(AS_THREADS) void k_as_offsets(Args g) {
    __shared__ int64_t lds[AS_THREADS / 64];
    if (g.counts[1] != PV_OK) {
        for (int64_t p = threadIdx.x; p <= g.n_pairs; p += AS_THREADS) g.pair_seg_off[p] = -1;
        return;
    }
    const Layout y = layout_of(g);
    const int64_t* pair_cnt = (const int64_t*)(g.scratch + y.pair_cnt);
    const int64_t total = block_scan_to(g.n_pairs, g.pair_seg_off, lds, [&](int64_t p) { return pair_cnt[2 * p]; });
    if (threadIdx.x == 0) g.counts[0] = total;
}

// where a slot's segment lives: false if the slot holds none
struct SegRef { int64_t pair, idx, out; SegSlot s; uint32_t* dirs; };
__device__ inline bool seg_of_slot(const Args& g, const Layout& y, int64_t slot, SegRef* r) {
    const int64_t* slot_off = slot_off_of(g);
    if (slot >= slot_off[g.n_pairs]) return false;
    const int64_t p = owner_of(slot_off, g.n_pairs, slot);
    const int64_t* pair_cnt = (const int64_t*)(g.scratch + y.pair_cnt);
    const int64_t idx = slot - slot_off[p];
    if (idx >= pair_cnt[2 * p]) return false;
    r->pair = p; r->idx = idx; r->out = g.pair_seg_off[p] + idx;
    r->s = ((const SegSlot*)(g.scratch + y.segs))[slot];
    // rows of the pair's earlier segments are fewer than a0, and each segment rounds its rows up to eight: 256 bytes a slot
    r->dirs = (uint32_t*)(g.scratch + y.dirs + 32 * (g.a_off[p] - g.a_off[0] + r->s.a0) + 256 * slot);
    return true;
}

__device__ inline int as_dlo(int64_t d) {
    const int ad = (int)(d < 0 ? -d : d);
    return (int)(d < 0 ? d : 0) - (AS_W - 1 - ad) / 2;
}

__device__ inline uint32_t umin32(uint32_t a, uint32_t b) { return a < b ? a : b; }

// one wavefront per segment; lane l holds band cells 2l and 2l + 1
__global__ __launch_bounds__(AS_THREADS) void k_as_sweep(Args g) {
    if (g.counts[1] != PV_OK) return;
    const Layout y = layout_of(g);
    const int lane = threadIdx.x & 63;
    const int64_t slot = (int64_t)blockIdx.x * (AS_THREADS / 64) + (threadIdx.x >> 6);
    SegRef r;
    if (!seg_of_slot(g, y, slot, &r)) return;
    const int64_t n = r.s.n, m = r.s.m, d = m - n;
    if (d > AS_DMAX || d < -AS_DMAX || n == 0) return;
    const uint8_t* A = g.A + g.a_off[r.pair] + r.s.a0;
    const uint8_t* B = g.B + g.b_off[r.pair] + r.s.b0;
    const int dlo = as_dlo(d);
    const int c0 = 2 * lane, c1 = c0 + 1;
    // row 0
    uint32_t h0, h1;
    {
        const int64_t j0 = dlo + c0, j1 = dlo + c1;
        h0 = j0 >= 0 && j0 <= m ? (uint32_t)j0 : AS_INF;
        h1 = j1 >= 0 && j1 <= m ? (uint32_t)j1 : AS_INF;
    }
    // the truth bytes under the lane's two cells in row 1: B[j - 1], j = 1 + dlo + c
    uint32_t bb0, bb1;
    {
        const int64_t q0 = dlo + c0, q1 = dlo + c1;
        bb0 = q0 >= 0 && q0 < m ? B[q0] : 0;
        bb1 = q1 >= 0 && q1 < m ? B[q1] : 0;
    }
    uint32_t word = 0;
    for (int64_t i0 = 1; i0 <= n; i0 += 64) {
        // the 64 assembly bytes of rows i0 .. i0+63, and the 64 truth bytes that enter the band at cell 127 behind them
        const int64_t qa = i0 - 1 + lane, qb = i0 + dlo + (AS_W - 1) + lane;
        const uint32_t ca = qa < n ? A[qa] : 0;
        const uint32_t cb = qb >= 0 && qb < m ? B[qb] : 0;
        const int rows = (int)min((int64_t)64, n - i0 + 1);
        for (int ri = 0; ri < rows; ri++) {
            const int64_t i = i0 + ri;
            const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)ca, ri);
            // cells with j >= 1: c >= 1 - (i + dlo); with 0 <= j <= m: -(i + dlo) <= c <= m - i - dlo
            const int64_t base = i + dlo;
            const int lo = (int)max((int64_t)-1, min((int64_t)AS_W + 1, -base));
            const int hi = (int)max((int64_t)-1, min((int64_t)AS_W + 1, m - base));
            const uint32_t up_next = __shfl_down(h0, 1, 64);
            const uint32_t dg0 = c0 > lo ? h0 + (a != bb0) : AS_INF, u0 = h1 + 1;
            const uint32_t dg1 = c1 > lo ? h1 + (a != bb1) : AS_INF, u1 = lane == 63 ? AS_INF : up_next + 1;
            uint32_t t0 = dg0 <= u0 ? dg0 : u0, t1 = dg1 <= u1 ? dg1 : u1;
            uint32_t dir0 = dg0 <= u0 ? DIR_DIAG : DIR_UP, dir1 = dg1 <= u1 ? DIR_DIAG : DIR_UP;
            if (c0 < lo || c0 > hi) t0 = AS_INF;
            if (c1 < lo || c1 > hi) t1 = AS_INF;
            // H[c] = min(T[c], min over c' < c of T[c'] + (c - c')): the prefix minimum of key[c'] = T[c'] + (128 - c')
            const uint32_t key0 = t0 + (uint32_t)(AS_W - c0), key1 = t1 + (uint32_t)(AS_W - c1);
            uint32_t x = umin32(key0, key1);
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) {
                const uint32_t z = __shfl_up(x, s, 64);
                if (lane >= s) x = umin32(x, z);
            }
            uint32_t e = __shfl_up(x, 1, 64);   // the cells of the lanes before this one
            if (lane == 0) e = 0xFFFFFFFFu;
            const uint32_t l0 = lane == 0 ? AS_INF + AS_W : e - (uint32_t)(AS_W - c0);
            const uint32_t l1 = umin32(e, key0) - (uint32_t)(AS_W - c1);
            if (l0 < t0) { t0 = l0; dir0 = DIR_LEFT; }
            if (l1 < t1) { t1 = l1; dir1 = DIR_LEFT; }
            h0 = c0 < lo || c0 > hi ? AS_INF : t0;
            h1 = c1 < lo || c1 > hi ? AS_INF : t1;
            word |= (dir0 | (dir1 << 2)) << (4 * ((i - 1) & 7));
            if (((i - 1) & 7) == 7 || i == n) {
                r.dirs[((i - 1) >> 3) * 64 + lane] = word;
                word = 0;
            }
            // the truth bytes of the next row: every cell takes its right neighbour's
            const uint32_t nb0 = __shfl_down(bb0, 1, 64);
            bb0 = bb1;
            bb1 = lane == 63 ? (uint32_t)__builtin_amdgcn_readlane((int)cb, ri) : nb0;
        }
    }
}

__device__ inline void poison_seg(pv_assess_seg* s) {
    int64_t* w = (int64_t*)s;
    for (int i = 0; i < 8; i++) w[i] = -1;
}

// the walk back from (n, m) by the stored directions, for the counting pass and the writing pass alike: the visitor sees every
// step with the i, j it leaves from. false: the walk left the band or the matrix (never expected; nothing is read outside).
//   v.diag(i, j, a, b)   A[a0+i-1] against B[b0+j-1]: a match or a substitution
//   v.up(i, j, x, hp)    an insertion of x = A[a0+i-1] before truth position b0+j
//   v.left(i, j, x, hp)  a deletion of x = B[b0+j-1] before assembly position a0+i
template <typename V>
__device__ inline bool as_walk(const SegRef& r, const uint8_t* Ac, const uint8_t* Bc, int64_t nb, int dlo, int32_t* edge_out,
                               V& v) {
    int64_t i = r.s.n, j = r.s.m, have = -1;
    uint32_t word = 0;
    int32_t edge = 0;
    bool broken = false;
    for (;;) {
        const int c = (int)(j - i - dlo);
        if (c < 0 || c >= AS_W || j < 0) { broken = true; break; }
        if (c == 0 || c == AS_W - 1) edge = 1;
        if (i == 0 && j == 0) break;
        int step = DIR_LEFT;
        if (i > 0) {
            const int64_t at = ((i - 1) >> 3) * 64 + (c >> 1);
            if (at != have) { word = r.dirs[at]; have = at; }
            step = (word >> (4 * ((i - 1) & 7) + 2 * (c & 1))) & 3;
        }
        if (j == 0 && step != DIR_UP) { broken = true; break; }
        if (step == DIR_DIAG) {
            v.diag(i, j, Ac[r.s.a0 + i - 1], Bc[r.s.b0 + j - 1]);
            i--; j--;
        } else if (step == DIR_UP) {
            const uint8_t x = Ac[r.s.a0 + i - 1];
            const int64_t q = r.s.b0 + j;
            v.up(i, j, x, (q - 1 >= 0 && Bc[q - 1] == x) || (q < nb && Bc[q] == x));
            i--;
        } else {
            const int64_t q = r.s.b0 + j - 1;
            const uint8_t x = Bc[q];
            v.left(i, j, x, (q - 1 >= 0 && Bc[q - 1] == x) || (q + 1 < nb && Bc[q + 1] == x));
            j--;
        }
    }
    *edge_out = edge;
    return !broken;
}

struct CountSteps {
    int32_t nm = 0, nsub = 0, nins = 0, ndel = 0, hpi = 0, hpd = 0;
    __device__ void diag(int64_t, int64_t, uint8_t a, uint8_t b) { if (a == b) nm++; else nsub++; }
    __device__ void up(int64_t, int64_t, uint8_t, bool hp) { nins++; hpi += hp; }
    __device__ void left(int64_t, int64_t, uint8_t, bool hp) { ndel++; hpd += hp; }
};

// one lane per slot: the walk back from (n, m), and the segment's record
__global__ __launch_bounds__(AS_THREADS) void k_as_trace(Args g) {
    const int64_t slot = (int64_t)blockIdx.x * AS_THREADS + threadIdx.x;
    if (g.counts[1] != PV_OK) {
        if (slot < g.seg_capacity) poison_seg(g.segs + slot);
        return;
    }
    const Layout y = layout_of(g);
    SegRef r;
    if (!seg_of_slot(g, y, slot, &r)) return;
    const int64_t n = r.s.n, m = r.s.m, d = m - n;
    const int64_t nb = g.b_off[r.pair + 1] - g.b_off[r.pair];
    pv_assess_seg o;
    memset(&o, 0, sizeof(o));
    o.a_start = r.s.a0; o.b_start = r.s.b0;
    o.n_rows = (int32_t)n; o.n_cols = (int32_t)m;
    o.pair = (int32_t)r.pair;
    // every segment but the pair's last ends at a kept anchor
    o.anchor = r.idx + 1 == ((const int64_t*)(g.scratch + y.pair_cnt))[2 * r.pair] ? 0 : AS_K;
    if (d > AS_DMAX || d < -AS_DMAX) {
        o.status = PV_ASSESS_SEG_UNALIGNED;
        g.segs[r.out] = o;
        return;
    }
    const uint8_t* Ac = g.A + g.a_off[r.pair];   // contig coordinates
    const uint8_t* Bc = g.B + g.b_off[r.pair];
    const int dlo = as_dlo(d);
    CountSteps v;
    int32_t edge = 0;
    const bool broken = !as_walk(r, Ac, Bc, nb, dlo, &edge, v);
    o.status = broken ? PV_ASSESS_SEG_BROKEN : PV_ASSESS_SEG_ALIGNED;
    o.edge = edge; o.match = v.nm; o.sub = v.nsub; o.ins = v.nins; o.del = v.ndel; o.hp_ins = v.hpi; o.hp_del = v.hpd;
    g.segs[r.out] = o;
}

// one workgroup per pair: its records -> totals[pair][16]
__global__ __launch_bounds__(AS_THREADS) void k_as_reduce(Args g) {
    __shared__ int64_t s_part[AS_THREADS / 64][12];
    const int64_t p = blockIdx.x;
    int64_t* out = g.totals + p * PV_ASSESS_TOTALS;
    if (g.counts[1] != PV_OK) {
        if (threadIdx.x < PV_ASSESS_TOTALS) out[threadIdx.x] = -1;
        return;
    }
    const Layout y = layout_of(g);
    const int64_t* pair_cnt = (const int64_t*)(g.scratch + y.pair_cnt);
    const int64_t s0 = g.pair_seg_off[p], ns = pair_cnt[2 * p];
    int64_t v[12];
    for (int f = 0; f < 12; f++) v[f] = 0;
    for (int64_t s = threadIdx.x; s < ns; s += AS_THREADS) {
        const pv_assess_seg x = g.segs[s0 + s];
        v[4] += x.anchor;
        if (x.status == PV_ASSESS_SEG_UNALIGNED) {
            v[2]++; v[10] += x.n_rows; v[11] += x.n_cols;
        } else {
            v[1]++; v[3] += x.edge;
            v[4] += x.match; v[5] += x.sub; v[6] += x.ins; v[7] += x.del; v[8] += x.hp_ins; v[9] += x.hp_del;
        }
    }
    for (int f = 0; f < 12; f++) v[f] = wave_sum(v[f]);
    if ((threadIdx.x & 63) == 0)
        for (int f = 0; f < 12; f++) s_part[threadIdx.x >> 6][f] = v[f];
    __syncthreads();
    if (threadIdx.x < PV_ASSESS_TOTALS) {
        const int f = threadIdx.x;
        int64_t t = 0;
        if (f == 0) t = ns;
        else if (f < 12) for (int w = 0; w < AS_THREADS / 64; w++) t += s_part[w][f];
        else if (f == 12) t = ns - 1;
        else if (f == 13) t = pair_cnt[2 * p + 1];
        out[f] = t;
    }
}

// the status is not PV_OK and known to the host alone (the scratch cannot hold even the slot offsets): poison everything
__global__ __launch_bounds__(AS_THREADS) void k_as_poison(Args g, int64_t need_scratch) {
    const int64_t t = (int64_t)blockIdx.x * AS_THREADS + threadIdx.x;
    if (t < g.seg_capacity) poison_seg(g.segs + t);
    if (t <= g.n_pairs) g.pair_seg_off[t] = -1;
    if (t < g.n_pairs * PV_ASSESS_TOTALS) g.totals[t] = -1;
    if (t == 0) {
        g.counts[0] = 0; g.counts[1] = PV_ERR_LIMIT; g.counts[2] = -1; g.counts[3] = need_scratch;
        if (g.with_err) { g.counts[4] = 0; g.counts[5] = -1; g.counts[6] = 0; g.counts[7] = 0; }
    }
}

// ---- pv_assess_errors_dev: the error records and the calibration table ---------------------------------------------------
// PV_ERR_CAPACITY is the one status under which the outputs (but errs) are still valid
__device__ inline bool as_failed(const Args& g) { return g.counts[1] != PV_OK && g.counts[1] != PV_ERR_CAPACITY; }

// one lane per slot: how many error records its segment gives
__global__ __launch_bounds__(AS_THREADS) void k_as_errcnt(Args g) {
    if (as_failed(g)) return;
    const int64_t slot = (int64_t)blockIdx.x * AS_THREADS + threadIdx.x;
    if (slot >= slot_off_of(g)[g.n_pairs]) return;
    const Layout y = layout_of(g);
    SegRef r;
    int64_t cnt = 0;
    if (seg_of_slot(g, y, slot, &r)) {
        const pv_assess_seg x = g.segs[r.out];
        if (x.status == PV_ASSESS_SEG_ALIGNED) cnt = (int64_t)x.sub + x.ins + x.del;
    }
    ((int64_t*)(g.scratch + y.err_cnt))[slot] = cnt;
}

// one block: the scan over all slots, pair_err_off, the need and the status
__global__ __launch_bounds__(AS_THREADS) void k_as_erroff(Args g, ErrArgs e) {
    __shared__ int64_t lds[AS_THREADS / 64];
    if (as_failed(g)) return;
    const Layout y = layout_of(g);
    const int64_t* slot_off = slot_off_of(g);
    const int64_t* err_cnt = (const int64_t*)(g.scratch + y.err_cnt);
    int64_t* err_off = (int64_t*)(g.scratch + y.err_off);
    const int64_t need = block_scan_to(slot_off[g.n_pairs], err_off, lds, [&](int64_t s) { return err_cnt[s]; });
    __syncthreads();   // err_off is complete
    for (int64_t p = threadIdx.x; p <= g.n_pairs; p += AS_THREADS) e.pair_err_off[p] = err_off[slot_off[p]];
    if (threadIdx.x == 0) {
        const bool fits = need <= e.err_capacity;
        g.counts[4] = fits ? need : 0;
        g.counts[5] = need;
        if (!fits) g.counts[1] = PV_ERR_CAPACITY;
    }
}

__device__ inline uint32_t as_q(uint8_t q) { return q > PV_ASSESS_QBINS - 1 ? PV_ASSESS_QBINS - 1 : q; }

// one workgroup per slot: the qualities of the segment's rows (if it is aligned) and of the anchor behind it -> the slot's
// partial table, its error columns zero (k_as_errors fills them)
__global__ __launch_bounds__(AS_THREADS) void k_as_hist(Args g, ErrArgs e) {
    __shared__ uint32_t s_tab[AS_QTAB];
    if (as_failed(g)) return;
    const Layout y = layout_of(g);
    const int64_t slot = blockIdx.x;
    SegRef r;
    if (!seg_of_slot(g, y, slot, &r)) return;   // (the same in every thread)
    for (int t = threadIdx.x; t < AS_QTAB; t += AS_THREADS) s_tab[t] = 0;
    __syncthreads();
    const pv_assess_seg x = g.segs[r.out];
    const uint8_t* Q = e.Q + g.a_off[r.pair];
    // the anchor lies directly behind the segment's rows: one contiguous range
    const int64_t lo = x.status == PV_ASSESS_SEG_ALIGNED ? r.s.a0 : r.s.a0 + r.s.n, hi = r.s.a0 + r.s.n + x.anchor;
    uint32_t cur = 0, run = 0;   // equal qualities in a row cost one LDS atomic
    for (int64_t k = lo + threadIdx.x; k < hi; k += AS_THREADS) {
        const uint32_t q = as_q(Q[k]);
        if (q != cur && run) { atomicAdd(&s_tab[4 * cur], run); run = 0; }
        cur = q;
        run++;
    }
    if (run) atomicAdd(&s_tab[4 * cur], run);
    __syncthreads();
    uint32_t* part = (uint32_t*)(g.scratch + y.qpart) + slot * AS_QTAB;
    for (int t = threadIdx.x; t < AS_QTAB; t += AS_THREADS) part[t] = s_tab[t];
}

// the writing pass: records from the end of the segment's range, since the walk runs backwards
struct WriteSteps {
    pv_assess_error* out;    // one past the next record to write; null: none is written
    const uint8_t* Q;        // the contig's qualities, or null
    uint32_t* part;          // the slot's partial table, or null
    int64_t a0, b0, na;
    int32_t pair, segment;
    __device__ void put(uint8_t kind, int64_t a_pos, int64_t b_pos, uint8_t a_base, uint8_t b_base, bool hp) {
        uint32_t q = 255;
        if (Q) {
            if (kind != PV_ASSESS_ERR_DEL) q = as_q(Q[a_pos]);
            else if (na == 0) q = 0;
            else {
                q = PV_ASSESS_QBINS - 1;
                if (a_pos - 1 >= 0) q = min(q, as_q(Q[a_pos - 1]));
                if (a_pos < na) q = min(q, as_q(Q[a_pos]));
            }
            part[4 * q + kind]++;   // this lane's own slot: nobody else writes it
        }
        if (!out) return;
        pv_assess_error x;
        x.a_pos = a_pos; x.b_pos = b_pos; x.pair = pair; x.segment = segment;
        x.kind = kind; x.a_base = a_base; x.b_base = b_base; x.hp = hp; x.qual = (uint8_t)q;
        x.pad[0] = x.pad[1] = x.pad[2] = 0;
        *--out = x;
    }
    __device__ void diag(int64_t i, int64_t j, uint8_t a, uint8_t b) {
        if (a != b) put(PV_ASSESS_ERR_SUB, a0 + i - 1, b0 + j - 1, a, b, false);
    }
    __device__ void up(int64_t i, int64_t j, uint8_t x, bool hp) { put(PV_ASSESS_ERR_INS, a0 + i - 1, b0 + j, x, 0, hp); }
    __device__ void left(int64_t i, int64_t j, uint8_t x, bool hp) { put(PV_ASSESS_ERR_DEL, a0 + i, b0 + j - 1, 0, x, hp); }
};

// one lane per slot: the walk again. Under PV_ERR_CAPACITY nothing is written, but the table still gets its errors.
__global__ __launch_bounds__(AS_THREADS) void k_as_errors(Args g, ErrArgs e) {
    if (as_failed(g)) return;
    const bool write = g.counts[1] == PV_OK;
    if (!write && !e.Q) return;
    const int64_t slot = (int64_t)blockIdx.x * AS_THREADS + threadIdx.x;
    const Layout y = layout_of(g);
    SegRef r;
    if (!seg_of_slot(g, y, slot, &r)) return;
    const int64_t* err_off = (const int64_t*)(g.scratch + y.err_off);
    const int64_t first = err_off[slot], last = err_off[slot + 1];
    if (first == last) return;   // no record: unaligned, broken or without an error
    WriteSteps v;
    v.out = write ? e.errs + last : nullptr;
    v.Q = e.Q ? e.Q + g.a_off[r.pair] : nullptr;
    v.part = e.Q ? (uint32_t*)(g.scratch + y.qpart) + slot * AS_QTAB : nullptr;
    v.a0 = r.s.a0; v.b0 = r.s.b0; v.na = g.a_off[r.pair + 1] - g.a_off[r.pair];
    v.pair = (int32_t)r.pair; v.segment = (int32_t)r.idx;
    int32_t edge;
    as_walk(r, g.A + g.a_off[r.pair], g.B + g.b_off[r.pair], g.b_off[r.pair + 1] - g.b_off[r.pair], as_dlo(r.s.m - r.s.n), &edge, v);
}

// one workgroup per pair: wave w sums the partial tables of the pair's segments w, w + 8, ..., a lane six entries of each; the
// eight sums are then added in the order of w
constexpr int QR_WAVES = 8, QR_PER = (AS_QTAB + 63) / 64;
__global__ __launch_bounds__(QR_WAVES * 64) void k_as_qreduce(Args g, ErrArgs e) {
    __shared__ int64_t s_sum[QR_WAVES][AS_QTAB];
    if (as_failed(g)) return;
    const Layout y = layout_of(g);
    const int64_t p = blockIdx.x;
    const int64_t ns = ((const int64_t*)(g.scratch + y.pair_cnt))[2 * p];
    const uint32_t* part = (const uint32_t*)(g.scratch + y.qpart) + slot_off_of(g)[p] * AS_QTAB;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int64_t acc[QR_PER];
#pragma unroll
    for (int k = 0; k < QR_PER; k++) acc[k] = 0;
    for (int64_t s = w; s < ns; s += QR_WAVES) {   // (asking for this loop to be unrolled by four made the kernel four times slower)
#pragma unroll
        for (int k = 0; k < QR_PER; k++) {
            const int t = lane + 64 * k;
            if (t < AS_QTAB) acc[k] += part[s * AS_QTAB + t];
        }
    }
#pragma unroll
    for (int k = 0; k < QR_PER; k++)
        if (lane + 64 * k < AS_QTAB) s_sum[w][lane + 64 * k] = acc[k];
    __syncthreads();
    for (int t = threadIdx.x; t < AS_QTAB; t += QR_WAVES * 64) {
        int64_t v = 0;
        for (int i = 0; i < QR_WAVES; i++) v += s_sum[i][t];
        e.qhist[p * AS_QTAB + t] = v;
    }
}

// PV_ERR_INVALID or PV_ERR_LIMIT: 0xFF over every new output
__global__ __launch_bounds__(AS_THREADS) void k_as_epoison(Args g, ErrArgs e) {
    if (!as_failed(g)) return;
    const int64_t t0 = (int64_t)blockIdx.x * AS_THREADS + threadIdx.x, step = (int64_t)gridDim.x * AS_THREADS;
    int64_t* w = (int64_t*)e.errs;
    for (int64_t t = t0; t < e.err_capacity * 4; t += step) w[t] = -1;
    for (int64_t t = t0; t <= g.n_pairs; t += step) e.pair_err_off[t] = -1;
    if (e.qhist)
        for (int64_t t = t0; t < g.n_pairs * AS_QTAB; t += step) e.qhist[t] = -1;
}

int assess_check(int64_t n_pairs, int segment, int max_shift, int64_t seg_capacity) {
    PV_CHECK(n_pairs >= 0 && seg_capacity >= 0, PV_ERR_INVALID, "assess: negative sizes");
    PV_CHECK(n_pairs < (1ll << 31) && seg_capacity < (1ll << 31), PV_ERR_LIMIT, "assess: too many pairs or segments for one launch");
    PV_CHECK(segment >= 256 && segment <= 65536 && segment % 32 == 0, PV_ERR_INVALID,
             "assess: segment must be a multiple of 32 in [256, 65536] (got %d)", segment);
    PV_CHECK(max_shift >= 32 && max_shift <= 1048576, PV_ERR_INVALID, "assess: max_shift must lie in [32, 1048576] (got %d)", max_shift);
    return PV_OK;
}

// the launches of pv_assess_dev and, with e, those of pv_assess_errors_dev behind them
int assess_launch(pv_ctx* ctx, const Args& g, const ErrArgs* e, hipStream_t st) {
    const int64_t n_pairs = g.n_pairs, seg_capacity = g.seg_capacity;
    pv_prof_scope ps_all(ctx, "assess", st);
    const int64_t most = std::max(std::max(seg_capacity, n_pairs * PV_ASSESS_TOTALS), n_pairs + 1);
    const int64_t head = as_layout(n_pairs, n_pairs, 0, g.with_err).total;   // the least any batch of n_pairs needs
    const unsigned per_slot = (unsigned)((seg_capacity + AS_THREADS - 1) / AS_THREADS);
    if (g.scratch_bytes < head) {
        k_as_poison<<<(unsigned)((most + AS_THREADS - 1) / AS_THREADS), AS_THREADS, 0, st>>>(g, head);
        if (e) k_as_epoison<<<1024, AS_THREADS, 0, st>>>(g, *e);
        PV_HIP(hipGetLastError());
        pv_set_error("assess: the scratch of %lld bytes cannot hold %lld pairs", (long long)g.scratch_bytes, (long long)n_pairs);
        return PV_ERR_LIMIT;
    }
    k_as_setup<<<1, AS_THREADS, 0, st>>>(g);
    if (seg_capacity > 0) { pv_prof_scope ps(ctx, "k_as_anchor", st); k_as_anchor<<<(unsigned)seg_capacity, AS_THREADS, 0, st>>>(g); }
    if (n_pairs > 0) k_as_chain<<<(unsigned)n_pairs, AS_THREADS, 0, st>>>(g);
    k_as_offsets<<<1, AS_THREADS, 0, st>>>(g);
    if (seg_capacity > 0) {
        {
            pv_prof_scope ps(ctx, "k_as_sweep", st);
            k_as_sweep<<<(unsigned)((seg_capacity + AS_THREADS / 64 - 1) / (AS_THREADS / 64)), AS_THREADS, 0, st>>>(g);
        }
        pv_prof_scope ps(ctx, "k_as_trace", st);
        k_as_trace<<<per_slot, AS_THREADS, 0, st>>>(g);
    }
    if (n_pairs > 0) k_as_reduce<<<(unsigned)n_pairs, AS_THREADS, 0, st>>>(g);
    if (e) {
        if (seg_capacity > 0) { pv_prof_scope ps(ctx, "k_as_errcnt", st); k_as_errcnt<<<per_slot, AS_THREADS, 0, st>>>(g); }
        { pv_prof_scope ps(ctx, "k_as_erroff", st); k_as_erroff<<<1, AS_THREADS, 0, st>>>(g, *e); }
        if (seg_capacity > 0) {
            if (e->Q) { pv_prof_scope ps(ctx, "k_as_hist", st); k_as_hist<<<(unsigned)seg_capacity, AS_THREADS, 0, st>>>(g, *e); }
            pv_prof_scope ps(ctx, "k_as_errors", st);
            k_as_errors<<<per_slot, AS_THREADS, 0, st>>>(g, *e);
        }
        if (e->Q && n_pairs > 0) {
            pv_prof_scope ps(ctx, "k_as_qreduce", st);
            k_as_qreduce<<<(unsigned)n_pairs, QR_WAVES * 64, 0, st>>>(g, *e);
        }
        k_as_epoison<<<1024, AS_THREADS, 0, st>>>(g, *e);
    }
    PV_HIP(hipGetLastError());
    return PV_OK;
}

int64_t scratch_bytes_of(int64_t n_pairs, const int64_t* a_off, int segment, int with_err) {
    if (n_pairs < 0 || (n_pairs > 0 && !a_off) || segment < 1) return PV_ERR_INVALID;
    int64_t slots = 0;
    for (int64_t p = 0; p < n_pairs; p++) {
        const int64_t na = a_off[p + 1] - a_off[p];
        if (na < 0) return PV_ERR_INVALID;
        slots += na / segment + 1;
    }
    return as_layout(n_pairs, slots, n_pairs ? a_off[n_pairs] - a_off[0] : 0, with_err).total;
}

// the refusals that pv_assess_dev and pv_assess_errors_dev share
int assess_dev_check(pv_ctx* ctx, const uint8_t* A, const int64_t* a_off, const uint8_t* B, const int64_t* b_off, int64_t n_pairs,
                     int segment, int max_shift, int64_t seg_capacity, pv_assess_seg* segs, int64_t* pair_seg_off, int64_t* totals,
                     void* scratch, int64_t scratch_bytes, int64_t* d_counts) {
    PV_CHECK(ctx && a_off && b_off && pair_seg_off && d_counts, PV_ERR_INVALID, "assess: null argument");
    PV_CHECK(scratch_bytes >= 0, PV_ERR_INVALID, "assess: negative sizes");
    int rc;
    if ((rc = assess_check(n_pairs, segment, max_shift, seg_capacity))) return rc;
    PV_CHECK(n_pairs == 0 || (A && B && totals), PV_ERR_INVALID, "assess: sequences or totals missing");
    PV_CHECK(seg_capacity == 0 || segs, PV_ERR_INVALID, "assess: segment records missing");
    PV_CHECK(scratch_bytes == 0 || scratch, PV_ERR_INVALID, "assess: scratch missing");
    PV_CHECK(((uintptr_t)scratch & 255) == 0 && ((uintptr_t)segs & 7) == 0, PV_ERR_INVALID,
             "assess: scratch must be aligned to 256 bytes and the records to 8");
    return PV_OK;
}

}  // namespace

extern "C" int64_t pv_assess_scratch_bytes(int64_t n_pairs, const int64_t* a_off, int segment) {
    return scratch_bytes_of(n_pairs, a_off, segment, 0);
}

extern "C" int64_t pv_assess_errors_scratch_bytes(int64_t n_pairs, const int64_t* a_off, int segment) {
    return scratch_bytes_of(n_pairs, a_off, segment, 1);
}

extern "C" int pv_assess_dev(pv_ctx* ctx, const uint8_t* A, const int64_t* a_off, const uint8_t* B, const int64_t* b_off,
                             int64_t n_pairs, int segment, int max_shift, int64_t seg_capacity, pv_assess_seg* segs,
                             int64_t* pair_seg_off, int64_t* totals, void* scratch, int64_t scratch_bytes, int64_t* d_counts,
                             void* stream) {
    int rc;
    if ((rc = assess_dev_check(ctx, A, a_off, B, b_off, n_pairs, segment, max_shift, seg_capacity, segs, pair_seg_off, totals,
                               scratch, scratch_bytes, d_counts)))
        return rc;
    PV_HIP(hipSetDevice(ctx->device));
    Args g = {A, a_off, B, b_off, n_pairs, segment, max_shift, seg_capacity, segs, pair_seg_off, totals, (uint8_t*)scratch,
              scratch_bytes, d_counts, 0};
    return assess_launch(ctx, g, nullptr, pv_pick_stream(ctx, stream));
}

extern "C" int pv_assess_errors_dev(pv_ctx* ctx, const uint8_t* A, const int64_t* a_off, const uint8_t* B, const int64_t* b_off,
                                    int64_t n_pairs, int segment, int max_shift, int64_t seg_capacity, pv_assess_seg* segs,
                                    int64_t* pair_seg_off, int64_t* totals, const uint8_t* Q, int64_t err_capacity,
                                    pv_assess_error* errs, int64_t* pair_err_off, int64_t* qhist, void* scratch,
                                    int64_t scratch_bytes, int64_t* d_counts, void* stream) {
    int rc;
    if ((rc = assess_dev_check(ctx, A, a_off, B, b_off, n_pairs, segment, max_shift, seg_capacity, segs, pair_seg_off, totals,
                               scratch, scratch_bytes, d_counts)))
        return rc;
    PV_CHECK(pair_err_off && err_capacity >= 0, PV_ERR_INVALID, "assess: error offsets missing or a negative capacity");
    PV_CHECK(err_capacity == 0 || errs, PV_ERR_INVALID, "assess: error records missing");
    PV_CHECK(((uintptr_t)errs & 7) == 0, PV_ERR_INVALID, "assess: the error records must be aligned to 8 bytes");
    PV_CHECK((Q != nullptr) == (qhist != nullptr), PV_ERR_INVALID,
             "assess: qualities and their table come together or not at all");
    PV_HIP(hipSetDevice(ctx->device));
    Args g = {A, a_off, B, b_off, n_pairs, segment, max_shift, seg_capacity, segs, pair_seg_off, totals, (uint8_t*)scratch,
              scratch_bytes, d_counts, 1};
    ErrArgs e = {Q, err_capacity, errs, pair_err_off, qhist};
    return assess_launch(ctx, g, &e, pv_pick_stream(ctx, stream));
}

extern "C" int pv_assess(pv_ctx* ctx, const uint8_t* A, const int64_t* a_off, const uint8_t* B, const int64_t* b_off,
                         int64_t n_pairs, int segment, int max_shift, int64_t seg_capacity, pv_assess_seg* segs,
                         int64_t* pair_seg_off, int64_t* totals, int64_t* counts) {
    PV_CHECK(ctx && a_off && b_off && pair_seg_off && counts, PV_ERR_INVALID, "assess: null argument");
    int rc;
    if ((rc = assess_check(n_pairs, segment, max_shift, seg_capacity))) return rc;
    PV_CHECK(n_pairs == 0 || (A && B && totals), PV_ERR_INVALID, "assess: sequences or totals missing");
    PV_CHECK(seg_capacity == 0 || segs, PV_ERR_INVALID, "assess: segment records missing");
    for (int64_t p = 0; p < n_pairs; p++) {
        const int64_t na = a_off[p + 1] - a_off[p], nb = b_off[p + 1] - b_off[p];
        PV_CHECK(na >= 0 && nb >= 0, PV_ERR_INVALID, "assess: the offsets of pair %lld decrease", (long long)p);
        PV_CHECK(na < (1ll << 31) && nb < (1ll << 31), PV_ERR_INVALID, "assess: pair %lld holds a contig of 2^31 bytes or more",
                 (long long)p);
    }
    PV_CHECK(a_off[0] == 0 && b_off[0] == 0, PV_ERR_INVALID, "assess: offsets must start at 0");
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t np = (size_t)n_pairs, cap = (size_t)seg_capacity;
    const size_t n_a = (size_t)a_off[n_pairs], n_b = (size_t)b_off[n_pairs];
    const int64_t need = pv_assess_scratch_bytes(n_pairs, a_off, segment);
    uint8_t *d_a = nullptr, *d_b = nullptr, *d_scratch = nullptr;
    int64_t *d_ao = nullptr, *d_bo = nullptr, *d_so = nullptr, *d_tot = nullptr, *d_counts = nullptr;
    pv_assess_seg* d_segs = nullptr;
    if ((rc = pv_get(ctx, "as.a", n_a > 0 ? n_a : 1, &d_a))) return rc;
    if ((rc = pv_get(ctx, "as.b", n_b > 0 ? n_b : 1, &d_b))) return rc;
    if ((rc = pv_get(ctx, "as.a_off", np + 1, &d_ao))) return rc;
    if ((rc = pv_get(ctx, "as.b_off", np + 1, &d_bo))) return rc;
    if ((rc = pv_get(ctx, "as.seg_off", np + 1, &d_so))) return rc;
    if ((rc = pv_get(ctx, "as.totals", np > 0 ? np * PV_ASSESS_TOTALS : 1, &d_tot))) return rc;
    if ((rc = pv_get(ctx, "as.segs", cap > 0 ? cap : 1, &d_segs))) return rc;
    if ((rc = pv_get(ctx, "as.scratch", (size_t)need, &d_scratch))) return rc;
    if ((rc = pv_get(ctx, "as.counts", (size_t)4, &d_counts))) return rc;
    if (n_a) PV_HIP(hipMemcpyAsync(d_a, A, n_a, hipMemcpyHostToDevice, st));
    if (n_b) PV_HIP(hipMemcpyAsync(d_b, B, n_b, hipMemcpyHostToDevice, st));
    PV_HIP(hipMemcpyAsync(d_ao, a_off, (np + 1) * 8, hipMemcpyHostToDevice, st));
    PV_HIP(hipMemcpyAsync(d_bo, b_off, (np + 1) * 8, hipMemcpyHostToDevice, st));
    rc = pv_assess_dev(ctx, d_a, d_ao, d_b, d_bo, n_pairs, segment, max_shift, seg_capacity, d_segs, d_so, d_tot, d_scratch, need,
                       d_counts, st);
    if (rc) return rc;
    PV_HIP(hipMemcpyAsync(counts, d_counts, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    PV_HIP(hipMemcpyAsync(pair_seg_off, d_so, (np + 1) * 8, hipMemcpyDeviceToHost, st));
    if (np) PV_HIP(hipMemcpyAsync(totals, d_tot, np * PV_ASSESS_TOTALS * 8, hipMemcpyDeviceToHost, st));
    PV_HIP(hipStreamSynchronize(st));
    const int64_t status = counts[1];
    // the records: all of them where the call failed (they are poisoned), else those written
    const size_t n_rec = status == PV_OK ? (size_t)counts[0] : cap;
    if (n_rec) {
        PV_HIP(hipMemcpyAsync(segs, d_segs, n_rec * sizeof(pv_assess_seg), hipMemcpyDeviceToHost, st));
        PV_HIP(hipStreamSynchronize(st));
    }
    PV_CHECK(status != PV_ERR_LIMIT, PV_ERR_LIMIT, "assess: %lld segment records needed, %lld given", (long long)counts[2],
             (long long)seg_capacity);
    PV_CHECK(status == PV_OK, (int)status, "assess: device status %lld", (long long)status);
    return PV_OK;
}

extern "C" int pv_assess_errors(pv_ctx* ctx, const uint8_t* A, const int64_t* a_off, const uint8_t* B, const int64_t* b_off,
                                int64_t n_pairs, int segment, int max_shift, int64_t seg_capacity, pv_assess_seg* segs,
                                int64_t* pair_seg_off, int64_t* totals, const uint8_t* Q, int64_t err_capacity,
                                pv_assess_error* errs, int64_t* pair_err_off, int64_t* qhist, int64_t* counts) {
    PV_CHECK(ctx && a_off && b_off && pair_seg_off && pair_err_off && counts, PV_ERR_INVALID, "assess: null argument");
    int rc;
    if ((rc = assess_check(n_pairs, segment, max_shift, seg_capacity))) return rc;
    PV_CHECK(n_pairs == 0 || (A && B && totals), PV_ERR_INVALID, "assess: sequences or totals missing");
    PV_CHECK(seg_capacity == 0 || segs, PV_ERR_INVALID, "assess: segment records missing");
    PV_CHECK(err_capacity >= 0 && (err_capacity == 0 || errs), PV_ERR_INVALID, "assess: error records missing");
    PV_CHECK(((uintptr_t)errs & 7) == 0, PV_ERR_INVALID, "assess: the error records must be aligned to 8 bytes");
    PV_CHECK((Q != nullptr) == (qhist != nullptr), PV_ERR_INVALID, "assess: qualities and their table come together or not at all");
    for (int64_t p = 0; p < n_pairs; p++) {
        const int64_t na = a_off[p + 1] - a_off[p], nb = b_off[p + 1] - b_off[p];
        PV_CHECK(na >= 0 && nb >= 0, PV_ERR_INVALID, "assess: the offsets of pair %lld decrease", (long long)p);
        PV_CHECK(na < (1ll << 31) && nb < (1ll << 31), PV_ERR_INVALID, "assess: pair %lld holds a contig of 2^31 bytes or more",
                 (long long)p);
    }
    PV_CHECK(a_off[0] == 0 && b_off[0] == 0, PV_ERR_INVALID, "assess: offsets must start at 0");
    const size_t np = (size_t)n_pairs, cap = (size_t)seg_capacity, ecap = (size_t)err_capacity;
    const size_t n_a = (size_t)a_off[n_pairs], n_b = (size_t)b_off[n_pairs];
    if (Q)
        for (size_t k = 0; k < n_a; k++)
            PV_CHECK(Q[k] < PV_ASSESS_QBINS, PV_ERR_INVALID, "assess: quality %d at byte %lld is above %d", (int)Q[k], (long long)k,
                     PV_ASSESS_QBINS - 1);
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int64_t need = pv_assess_errors_scratch_bytes(n_pairs, a_off, segment);
    uint8_t *d_a = nullptr, *d_b = nullptr, *d_q = nullptr, *d_scratch = nullptr;
    int64_t *d_ao = nullptr, *d_bo = nullptr, *d_so = nullptr, *d_tot = nullptr, *d_eo = nullptr, *d_qh = nullptr, *d_counts = nullptr;
    pv_assess_seg* d_segs = nullptr;
    pv_assess_error* d_errs = nullptr;
    if ((rc = pv_get(ctx, "as.a", n_a > 0 ? n_a : 1, &d_a))) return rc;
    if ((rc = pv_get(ctx, "as.b", n_b > 0 ? n_b : 1, &d_b))) return rc;
    if ((rc = pv_get(ctx, "as.q", n_a > 0 ? n_a : 1, &d_q))) return rc;
    if ((rc = pv_get(ctx, "as.a_off", np + 1, &d_ao))) return rc;
    if ((rc = pv_get(ctx, "as.b_off", np + 1, &d_bo))) return rc;
    if ((rc = pv_get(ctx, "as.seg_off", np + 1, &d_so))) return rc;
    if ((rc = pv_get(ctx, "as.err_off", np + 1, &d_eo))) return rc;
    if ((rc = pv_get(ctx, "as.totals", np > 0 ? np * PV_ASSESS_TOTALS : 1, &d_tot))) return rc;
    if ((rc = pv_get(ctx, "as.qhist", np > 0 ? np * AS_QTAB : 1, &d_qh))) return rc;
    if ((rc = pv_get(ctx, "as.segs", cap > 0 ? cap : 1, &d_segs))) return rc;
    if ((rc = pv_get(ctx, "as.errs", ecap > 0 ? ecap : 1, &d_errs))) return rc;
    if ((rc = pv_get(ctx, "as.scratch", (size_t)need, &d_scratch))) return rc;
    if ((rc = pv_get(ctx, "as.counts", (size_t)8, &d_counts))) return rc;
    if (n_a) PV_HIP(hipMemcpyAsync(d_a, A, n_a, hipMemcpyHostToDevice, st));
    if (n_b) PV_HIP(hipMemcpyAsync(d_b, B, n_b, hipMemcpyHostToDevice, st));
    if (n_a && Q) PV_HIP(hipMemcpyAsync(d_q, Q, n_a, hipMemcpyHostToDevice, st));
    PV_HIP(hipMemcpyAsync(d_ao, a_off, (np + 1) * 8, hipMemcpyHostToDevice, st));
    PV_HIP(hipMemcpyAsync(d_bo, b_off, (np + 1) * 8, hipMemcpyHostToDevice, st));
    rc = pv_assess_errors_dev(ctx, d_a, d_ao, d_b, d_bo, n_pairs, segment, max_shift, seg_capacity, d_segs, d_so, d_tot,
                              Q ? d_q : nullptr, err_capacity, d_errs, d_eo, Q ? d_qh : nullptr, d_scratch, need, d_counts, st);
    if (rc) return rc;
    PV_HIP(hipMemcpyAsync(counts, d_counts, 8 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    PV_HIP(hipMemcpyAsync(pair_seg_off, d_so, (np + 1) * 8, hipMemcpyDeviceToHost, st));
    PV_HIP(hipMemcpyAsync(pair_err_off, d_eo, (np + 1) * 8, hipMemcpyDeviceToHost, st));
    if (np) PV_HIP(hipMemcpyAsync(totals, d_tot, np * PV_ASSESS_TOTALS * 8, hipMemcpyDeviceToHost, st));
    if (np && Q) PV_HIP(hipMemcpyAsync(qhist, d_qh, np * AS_QTAB * 8, hipMemcpyDeviceToHost, st));
    PV_HIP(hipStreamSynchronize(st));
    const int64_t status = counts[1];
    const bool valid = status == PV_OK || status == PV_ERR_CAPACITY;
    // the records: all of them where the call failed (they are poisoned), else those written; under PV_ERR_CAPACITY no error
    // record was written and the caller's stay as they were
    const size_t n_rec = valid ? (size_t)counts[0] : cap;
    const size_t n_err = status == PV_OK ? (size_t)counts[4] : valid ? 0 : ecap;
    if (n_rec) PV_HIP(hipMemcpyAsync(segs, d_segs, n_rec * sizeof(pv_assess_seg), hipMemcpyDeviceToHost, st));
    if (n_err) PV_HIP(hipMemcpyAsync(errs, d_errs, n_err * sizeof(pv_assess_error), hipMemcpyDeviceToHost, st));
    if (n_rec || n_err) PV_HIP(hipStreamSynchronize(st));
    PV_CHECK(status != PV_ERR_LIMIT, PV_ERR_LIMIT, "assess: %lld segment records needed, %lld given", (long long)counts[2],
             (long long)seg_capacity);
    PV_CHECK(status != PV_ERR_CAPACITY, PV_ERR_CAPACITY, "assess: %lld error records needed, %lld given", (long long)counts[5],
             (long long)err_capacity);
    PV_CHECK(status == PV_OK, (int)status, "assess: device status %lld", (long long)status);
    return PV_OK;
}
