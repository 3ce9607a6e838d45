// polish_realign.hip — the polisher's read realignment (every read re-aligned to the draft before the images are built).
//
// Restates ReadAligner::align_reads_to_reference (pepper/modules/src/local_reassembly/simple_aligner.cpp:66-107) over the
// striped Smith-Waterman of ssw.c / ssw_cpp.cpp with Aligner(match 4, mismatch 6, gap open 8, gap extend 2), the default
// Filter and maskLen 0. Per read of region g (window = win[win_off[g] .. win_off[g+1]), the draft from the region start):
//   pos < ref_start: dropped (no cigar words); otherwise the query (the read's bases) is aligned against window[pos-start:];
//   score > 1: new cigar ('=' / 'X' runs -> MATCH kept apart, S, I, D) and pos + ref_begin; else the read is kept as it was.
// Pinned where the reference is undefined: an empty query or an empty window keeps the read; a byte >= 128 is code 4.
//
// Kernels (all asynchronous on one stream, no host read-back):
//   k_rl_score<false>  one wavefront per read: local affine DP, the query cut into 64 lane strips (S rows each, H/E/code of
//                      a row packed in one LDS word), reference columns swept with an anti-diagonal skew (lane l works on
//                      column t - l at step t and hands its strip's bottom H and F to lane l + 1 through a shuffle).
//                      (max, first column, smallest row) per lane in visiting order, reduced lexicographically over the wave.
//   k_rl_score<true>   the same on the reversed query prefix [0, query_end] against columns ref_end .. 0; it stops, wave-
//                      uniformly, once every lane has passed the first column whose maximum reaches the score.
//   k_rl_bandw         ssw.c banded_sw, score only: one wavefront per read, lanes across the band of a query row (the F
//                      recurrence of a row by a prefix max), h_b / e_b / h_c rows in LDS; the band doubles until its maximum
//                      reaches the score.
//   k_rl_band          the pass at that width again, storing a 4-bit direction code per cell, then lane 0 traces back.
//                      Direction bytes come from a bounded scratch pool: tier k runs pool / slot_k workers (slots 192 KB,
//                      1 MB, 16 MB, the whole pool) that take reads in turn (the
//                      slicing), a read too large for tier k waits for tier k + 1, one too large for the whole pool is
//                      PV_ERR_LIMIT.
//   k_rl_scan          one block: cigar words per read -> exclusive offsets, status, counters.
//   k_rl_write         one wavefront per read: positions, cigar words (new or the input's), per-read records.
#include "pv_common.hpp"

namespace {

constexpr int RL_MATCH = 4, RL_MISMATCH = 6, RL_GAP_O = 8, RL_GAP_E = 2;
constexpr int RL_MAX_STRIP = 256;        // rows per lane: queries up to 16384 bases (64 KB of LDS)
constexpr int RL_MAX_WINDOW = 2047;      // H and E of a row are 13-bit fields: |H| <= 4 * window
constexpr int RL_BAND_THREADS = 64;
constexpr int RL_SCAN_THREADS = 1024;
enum { ST_UNCHANGED = 0, ST_REALIGNED = 1, ST_DROPPED = 2 };
enum { BAD_NONE = 0, BAD_LIMIT = 1, BAD_TRACE = 2 };

struct RlArgs {
    // input batch (device pointers)
    int n_regions;
    int64_t n_reads;
    const int64_t* ref_start;
    const int64_t* read_off;
    const int64_t* read_pos;
    const int64_t* base_off;
    const uint8_t* bases;
    const int64_t* cigar_off;
    const uint32_t* cigar;
    const int64_t* win_off;
    const uint8_t* win;
    // per-read scratch
    int32_t* res;        // [n_reads][6] score, ref_begin, ref_end, query_begin, query_end, band width
    uint8_t* state;      // [n_reads]
    uint8_t* bad;        // [n_reads] BAD_*
    int32_t* n_new;      // [n_reads] new cigar words (realigned reads)
    int64_t* cnt;        // [n_reads] output words per read
    uint32_t* tmp_cigar; // 2 * (base_off[r] - base_off[0]) + 2 * r: room for 2 * qlen + 2 words per read
    uint8_t* pool;       // direction bytes + raw traceback words
    int64_t pool_bytes;
    // output
    int64_t* out_pos;
    int64_t* out_cigar_off;
    uint32_t* out_cigar;
    int64_t cigar_cap;
    int32_t* out_score;
    int32_t* out_ends;
    uint8_t* out_state;
    int32_t* out_band;
    int64_t* counts;
};

__device__ __forceinline__ int rl_code(uint8_t b) {
    switch (b) {
        case 'A': case 'a': case 'U': case 'u': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': return 3;
        default: return 4;
    }
}

__device__ __forceinline__ int rl_score(int a, int b) { return (a == b && a < 4) ? RL_MATCH : -RL_MISMATCH; }

__device__ inline int rl_region_of(const RlArgs& a, int64_t r) {
    int lo = 0, hi = a.n_regions - 1;   // last g with read_off[g] <= r
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.read_off[mid] <= r) lo = mid; else hi = mid - 1;
    }
    return lo;
}

struct ReadView {
    const uint8_t* ref;   // window from the read's pos
    const uint8_t* q;
    int rlen, qlen;
};

__device__ inline ReadView rl_view(const RlArgs& a, int64_t r) {
    const int g = rl_region_of(a, r);
    const int64_t off = a.read_pos[r] - a.ref_start[g];
    const int64_t wlen = a.win_off[g + 1] - a.win_off[g];
    ReadView v;
    v.ref = a.win + a.win_off[g] + off;
    v.rlen = (int)(wlen - off);
    v.q = a.bases + a.base_off[r];
    v.qlen = (int)(a.base_off[r + 1] - a.base_off[r]);
    return v;
}

// H (13 bits) | E (13 bits) << 13 | query code (3 bits) << 26
__device__ __forceinline__ uint32_t pk(int h, int e, int qc) { return (uint32_t)h | ((uint32_t)e << 13) | ((uint32_t)qc << 26); }

// REV = false: the forward pass of every read (decides dropped / unchanged, writes score, ref_end, query_end).
// REV = true: reads with score > 1; writes ref_begin, query_begin.
template <bool REV>
__global__ __launch_bounds__(64) void k_rl_score(RlArgs a, int strip) {
    extern __shared__ uint32_t rows[];   // [strip][64]
    const int64_t r = blockIdx.x;
    const int lane = threadIdx.x;
    int rlen, qlen, term = 0, re = 0, qe = 0;
    const uint8_t *ref, *q;
    if (!REV) {
        const int g = rl_region_of(a, r);
        const int64_t pos = a.read_pos[r], start = a.ref_start[g];
        const int64_t wlen = a.win_off[g + 1] - a.win_off[g];
        const int64_t qn = a.base_off[r + 1] - a.base_off[r];
        int st = ST_UNCHANGED, bad = BAD_NONE;
        if (pos < start) st = ST_DROPPED;
        else if (pos - start >= wlen || qn == 0) st = ST_UNCHANGED;
        else if (qn > (int64_t)strip * 64 || wlen - (pos - start) > RL_MAX_WINDOW) bad = BAD_LIMIT;
        else st = -1;
        if (st >= 0 || bad) {
            if (lane == 0) {
                a.state[r] = (uint8_t)st;
                a.bad[r] = (uint8_t)bad;
                for (int k = 0; k < 6; k++) a.res[r * 6 + k] = 0;
            }
            return;
        }
        const ReadView v = rl_view(a, r);
        ref = v.ref; q = v.q; rlen = v.rlen; qlen = v.qlen;
    } else {
        if (a.state[r] != ST_REALIGNED) return;
        const ReadView v = rl_view(a, r);
        term = a.res[r * 6 + 0]; re = a.res[r * 6 + 2]; qe = a.res[r * 6 + 4];
        ref = v.ref; q = v.q; rlen = re + 1; qlen = qe + 1;
    }
    const int S = (qlen + 63) >> 6;            // rows per lane
    const int nl = (qlen + S - 1) / S;         // lanes with rows
    const int r0 = lane * S;
    const int nk = lane < nl ? min(S, qlen - r0) : 0;
    for (int k = 0; k < nk; k++) {
        const int qi = REV ? qe - (r0 + k) : r0 + k;
        rows[k * 64 + lane] = pk(0, 0, rl_code(q[qi]));
    }
    __syncthreads();
    int hbot = 0, fbot = 0, diag_prev = 0;
    int best = 0, bc = -1, br = qlen - 1;      // forward: (max, first column, smallest row); reverse: first hit of term
    const int T = rlen + nl - 1;
    for (int t = 0; t < T; t++) {
        const int up_h = __shfl_up(hbot, 1, 64), up_f = __shfl_up(fbot, 1, 64);
        const int c = t - lane;
        if (nk > 0 && c >= 0 && c < rlen) {
            int hd = lane == 0 ? 0 : diag_prev;
            int f = lane == 0 ? 0 : up_f;
            const int rc = rl_code(ref[REV ? re - c : c]);
            int h = 0;
            for (int k = 0; k < nk; k++) {
                const uint32_t w = rows[k * 64 + lane];
                const int ho = (int)(w & 8191u), eo = (int)((w >> 13) & 8191u), qc = (int)(w >> 26);
                const int e = max(max(eo - RL_GAP_E, ho - RL_GAP_O), 0);
                h = max(max(hd + rl_score(qc, rc), e), max(f, 0));
                hd = ho;
                rows[k * 64 + lane] = pk(h, e, qc);
                if (!REV) {
                    if (h > best) { best = h; bc = c; br = r0 + k; }
                } else if (h == term && bc < 0) {
                    bc = c; br = r0 + k;
                }
                f = max(max(f - RL_GAP_E, h - RL_GAP_O), 0);
            }
            hbot = h; fbot = f;
            diag_prev = up_h;
        } else if (c < 0) {
            diag_prev = 0;
        }
        if (REV && (t & 15) == 15) {
            int m = bc >= 0 ? bc : INT32_MAX;
            for (int d = 32; d >= 1; d >>= 1) m = min(m, __shfl_xor(m, d, 64));
            if (m != INT32_MAX && t - (nl - 1) >= m) break;   // every lane is past column m
        }
    }
    if (!REV) {
        // lexicographic: larger score, then smaller column, then smaller row
        for (int d = 32; d >= 1; d >>= 1) {
            const int ob = __shfl_xor(best, d, 64), oc = __shfl_xor(bc, d, 64), orr = __shfl_xor(br, d, 64);
            const bool take = ob > best || (ob == best && (oc < bc || (oc == bc && orr < br)));
            if (take) { best = ob; bc = oc; br = orr; }
        }
        if (lane == 0) {
            a.bad[r] = BAD_NONE;
            a.state[r] = best > 1 ? ST_REALIGNED : ST_UNCHANGED;
            a.res[r * 6 + 0] = best;
            a.res[r * 6 + 1] = 0;
            a.res[r * 6 + 2] = best > 1 ? bc : 0;
            a.res[r * 6 + 3] = 0;
            a.res[r * 6 + 4] = best > 1 ? br : 0;
            a.res[r * 6 + 5] = 0;
        }
    } else {
        int m = bc >= 0 ? bc : INT32_MAX, mr = bc >= 0 ? br : INT32_MAX;
        for (int d = 32; d >= 1; d >>= 1) {
            const int om = __shfl_xor(m, d, 64), orr = __shfl_xor(mr, d, 64);
            if (om < m || (om == m && orr < mr)) { m = om; mr = orr; }
        }
        if (lane == 0) {
            if (m == INT32_MAX) {   // the reverse pass always meets the score; anything else is reported, not used
                a.bad[r] = BAD_TRACE;
            } else {
                a.res[r * 6 + 1] = re - m;
                a.res[r * 6 + 3] = qe - mr;
            }
        }
    }
}

// ---- banded global pass (ssw.c banded_sw) ----

__device__ __forceinline__ int wave_incl_max(int v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(v, d, 64);
        if (lane >= d) v = max(v, y);
    }
    return v;
}

struct Band {
    const uint8_t* ref;   // ref_begin .. ref_end
    const uint8_t* q;     // query_begin .. query_end
    int rspan, qspan, score;
};

// One pass of width w over the band; rows h_b, e_b, h_c in LDS (rspan + 2 int16 each: 0 <= H <= 4 * 2047, E >= -8).
// dir != nullptr: one 4-bit direction code per cell, two cells per byte, rows of bwb = (bw + 1) / 2 bytes:
// nibble (j - x) of row i = (dh == 1) | (e1 > f1) << 1 | (de == 3) << 2 | (df == 5) << 3, which restates ssw.c's three codes.
// Returns the band maximum (wave-uniform).
__device__ int band_pass(const Band& b, int w, int16_t* h_b, int16_t* e_b, int16_t* h_c, uint8_t* dir, int bw) {
    const int lane = threadIdx.x;
    const int width = 2 * w + 3;
    const int asz = min(width, b.rspan + 2);
    for (int k = lane; k < asz; k += 64) { h_b[k] = 0; e_b[k] = 0; h_c[k] = 0; }
    __syncthreads();
    int mx = 0;
    for (int i = 0; i < b.qspan; i++) {
        const int x = max(i - w, 0), xp = max(i - 1 - w, 0);
        const int beg = x, end = min(b.rspan - 1, i + w);
        const int edge = min(end + 1, width - 1);
        if (lane == 0) { h_b[0] = 0; e_b[0] = 0; h_b[edge] = 0; e_b[edge] = 0; h_c[0] = 0; }
        __syncthreads();
        const int qc = rl_code(b.q[i]);
        int carry_g = 2 * beg - 2, carry_h = 0, carry_f = 0;
        for (int base = beg; base <= end; base += 64) {
            const int j = base + lane;
            const bool act = j <= end;
            int E = 0, de3 = 0, diag = 0, e1 = 0, G = INT32_MIN / 2;
            if (act) {
                const int e = j - xp + 1, d = j - xp;
                const int t1 = i == 0 ? -RL_GAP_O : h_b[e] - RL_GAP_O;
                const int t2 = i == 0 ? -RL_GAP_E : e_b[e] - RL_GAP_E;
                E = t1 > t2 ? t1 : t2;
                de3 = t1 > t2;
                diag = h_b[d] + rl_score(rl_code(b.ref[j]), qc);
                e1 = E > 0 ? E : 0;
                G = max(e1, diag) + 2 * j - 6;
            }
            const int incl = wave_incl_max(G);
            int excl = __shfl_up(incl, 1, 64);
            if (lane == 0) excl = INT32_MIN / 2;
            const int f = max(carry_g, excl) - 2 * j;          // F of cell j (exact: see DESIGN.md)
            const int f1 = f > 0 ? f : 0;
            const int t1 = e1 > f1 ? e1 : f1;
            const int hc = t1 > diag ? t1 : diag;
            int ph = __shfl_up(hc, 1, 64), pf = __shfl_up(f, 1, 64);
            if (lane == 0) { ph = carry_h; pf = carry_f; }
            const int df5 = (ph - RL_GAP_O) > (pf - RL_GAP_E);
            __syncthreads();   // every lane has read e_b[e] of this chunk before any lane writes e_b[u]
            const int code = (t1 <= diag) | ((e1 > f1) << 1) | (de3 << 2) | (df5 << 3);
            const int hi = __shfl_down(code, 1, 64);   // j - x = 64 k + lane: even lanes write their pair's byte
            if (act) {
                const int u = j - x + 1;
                e_b[u] = (int16_t)E;
                h_c[u] = (int16_t)hc;
                mx = max(mx, hc);
                if (dir && !(lane & 1)) dir[(int64_t)i * bw + ((j - x) >> 1)] = (uint8_t)(code | (hi << 4));
            }
            carry_g = max(carry_g, __shfl(incl, 63, 64));
            const int last = min(63, end - base);
            carry_h = __shfl(hc, last, 64);
            carry_f = __shfl(f, last, 64);
        }
        __syncthreads();
        const int ulast = end - x + 1;
        for (int k = 1 + lane; k <= ulast; k += 64) h_b[k] = h_c[k];
        __syncthreads();
    }
    for (int d = 32; d >= 1; d >>= 1) mx = max(mx, __shfl_xor(mx, d, 64));
    return mx;
}

// bytes per direction row
__device__ __forceinline__ int band_row_bytes(int rspan, int w) { return (min(2 * w + 1, rspan) + 1) >> 1; }

__device__ __forceinline__ int64_t band_need(int qspan, int rspan, int w) {
    const int64_t dir = ((int64_t)qspan * band_row_bytes(rspan, w) + 15) & ~(int64_t)15;
    return dir + 4 * ((int64_t)qspan + rspan + 4);
}

// banded_sw's traceback from the last cell: raw[0..n) = its ops (0 M, 1 I, 2 D; BAM packing) in forward order; returns n,
// or -1 when the trace leaves the band.
__device__ int band_traceback(const Band& b, int w, const uint8_t* dir, int bwb, uint32_t* raw) {
    const int bw = min(2 * w + 1, b.rspan);
    int n = 0, i = b.qspan - 1, j = b.rspan - 1, e = 0, state = 2;
    int op = 0, prev = 0;
    while (i > 0) {
        const int x = max(i - w, 0);
        if (j - x < 0 || j - x >= bw) return -1;
        const int v = (dir[(int64_t)i * bwb + ((j - x) >> 1)] >> (((j - x) & 1) << 2)) & 15;
        const int de = (v & 4) ? 3 : 2, df = (v & 8) ? 5 : 4;
        const int c = state == 2 ? ((v & 1) ? 1 : (v & 2) ? de : df) : state == 0 ? de : df;
        switch (c) {
            case 1: --i; --j; state = 2; op = 0; break;
            case 2: --i; state = 0; op = 1; break;
            case 3: --i; state = 2; op = 1; break;
            case 4: --j; state = 1; op = 2; break;
            case 5: --j; state = 2; op = 2; break;
            default: return -1;
        }
        if (op == prev) ++e;
        else { raw[n++] = ((uint32_t)e << 4) | (uint32_t)prev; prev = op; e = 1; }
    }
    if (op == 0) raw[n++] = ((uint32_t)(e + 1) << 4);
    else { raw[n++] = ((uint32_t)e << 4) | (uint32_t)op; raw[n++] = 1u << 4; }
    for (int s = 0, t = n - 1; s < t; s++, t--) { const uint32_t y = raw[s]; raw[s] = raw[t]; raw[t] = y; }
    return n;
}

// raw ops -> the read's new cigar: S head, M split into runs of '=' / 'X' (both op 0, kept apart), I, D, S tail
__device__ int emit_cigar(const ReadView& v, int rb, int qb, int qe, const uint32_t* raw, int nr, uint32_t* out) {
    int n = 0;
    if (qb > 0) out[n++] = ((uint32_t)qb << 4) | 4u;
    int ri = rb, qi = qb, run = 0, run_eq = -1;
    for (int k = 0; k < nr; k++) {
        const int op = (int)(raw[k] & 15), len = (int)(raw[k] >> 4);
        if (op == 0) {
            for (int t = 0; t < len; t++, ri++, qi++) {
                const int eq = rl_code(v.ref[ri]) == rl_code(v.q[qi]);
                if (eq != run_eq && run > 0) { out[n++] = (uint32_t)run << 4; run = 0; }
                run_eq = eq; run++;
            }
        } else {
            if (run > 0) { out[n++] = (uint32_t)run << 4; run = 0; }
            out[n++] = raw[k];
            if (op == 1) qi += len; else ri += len;
        }
    }
    if (run > 0) out[n++] = (uint32_t)run << 4;
    const int tail = v.qlen - qe - 1;
    if (tail > 0) out[n++] = ((uint32_t)tail << 4) | 4u;
    return n;
}

__device__ inline bool band_of(const RlArgs& a, int64_t r, ReadView& v, Band& b) {
    v = rl_view(a, r);
    const int32_t* rs = a.res + r * 6;
    const int score = rs[0], rb = rs[1], re = rs[2], qb = rs[3], qe = rs[4];
    if (!(0 <= rb && rb <= re && re < v.rlen && 0 <= qb && qb <= qe && qe < v.qlen)) return false;
    b.ref = v.ref + rb; b.q = v.q + qb; b.rspan = re - rb + 1; b.qspan = qe - qb + 1; b.score = score;
    return true;
}

// one wavefront per read: the score-only banded passes (no scratch), band doubling until its maximum reaches the score
__global__ __launch_bounds__(RL_BAND_THREADS) void k_rl_bandw(RlArgs a) {
    extern __shared__ int16_t bandw_rows[];
    const int64_t r = blockIdx.x;
    const int lane = threadIdx.x;
    if (a.state[r] != ST_REALIGNED || a.bad[r] != BAD_NONE) return;
    ReadView v;
    Band b;
    if (!band_of(a, r, v, b)) {
        if (lane == 0) { a.bad[r] = BAD_TRACE; a.n_new[r] = 0; }
        return;
    }
    int16_t* h_b = bandw_rows;
    int16_t* e_b = h_b + (b.rspan + 2);
    int16_t* h_c = e_b + (b.rspan + 2);
    int w = abs(b.rspan - b.qspan) + 1, mx;
    while ((mx = band_pass(b, w, h_b, e_b, h_c, nullptr, 0)) < b.score && w <= b.rspan + b.qspan) w *= 2;
    if (lane == 0) {
        if (mx < b.score) { a.bad[r] = BAD_TRACE; a.n_new[r] = 0; }   // a band over the whole matrix holds the optimum
        else a.res[r * 6 + 5] = w;
    }
}

// tier: workers = gridDim.x wavefronts, each owning `slot` bytes of the pool; reads r = worker, worker + workers, ...
__global__ __launch_bounds__(RL_BAND_THREADS) void k_rl_band(RlArgs a, int64_t slot, int last_tier) {
    extern __shared__ int16_t band_rows[];
    const int lane = threadIdx.x;
    uint8_t* my = a.pool + (int64_t)blockIdx.x * slot;
    for (int64_t r = blockIdx.x; r < a.n_reads; r += gridDim.x) {
        if (a.state[r] != ST_REALIGNED || a.bad[r] != BAD_NONE || a.n_new[r] >= 0) continue;
        ReadView v;
        Band b;
        if (!band_of(a, r, v, b)) continue;   // (k_rl_bandw flagged it)
        const int32_t* rs = a.res + r * 6;
        const int rb = rs[1], qb = rs[3], qe = rs[4];
        int16_t* h_b = band_rows;
        int16_t* e_b = h_b + (b.rspan + 2);
        int16_t* h_c = e_b + (b.rspan + 2);
        const int w = rs[5];
        const int64_t need = band_need(b.qspan, b.rspan, w);
        if (need > slot) {
            if (last_tier && lane == 0) a.bad[r] = BAD_LIMIT;
            continue;
        }
        const int bwb = band_row_bytes(b.rspan, w);
        uint8_t* dir = my;
        uint32_t* raw = (uint32_t*)(my + (((int64_t)b.qspan * bwb + 15) & ~(int64_t)15));
        band_pass(b, w, h_b, e_b, h_c, dir, bwb);
        __threadfence_block();
        __syncthreads();
        if (lane == 0) {
            const int nr = band_traceback(b, w, dir, bwb, raw);
            if (nr < 0) {
                a.bad[r] = BAD_TRACE;
                a.n_new[r] = 0;
            } else {
                uint32_t* out = a.tmp_cigar + 2 * (a.base_off[r] - a.base_off[0]) + 2 * r;
                a.n_new[r] = emit_cigar(v, rb, qb, qe, raw, nr, out);
            }
        }
        __syncthreads();
    }
}

__global__ void k_rl_count(RlArgs a) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n_reads) return;
    const int st = a.state[r];
    a.cnt[r] = st == ST_DROPPED ? 0 : (st == ST_REALIGNED ? (int64_t)max(a.n_new[r], 0) : a.cigar_off[r + 1] - a.cigar_off[r]);
}

template <typename T>
__device__ inline T block_excl_sum(T v, T* lds, T* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    T x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) lds[w] = x;
    __syncthreads();
    T off = 0, sum = 0;
    for (int i = 0; i < RL_SCAN_THREADS / 64; i++) {
        off += i < w ? lds[i] : 0;
        sum += lds[i];
    }
    __syncthreads();
    *total = sum;
    return off + x - v;
}

__global__ __launch_bounds__(RL_SCAN_THREADS) void k_rl_scan(RlArgs a) {
    __shared__ int64_t lds[RL_SCAN_THREADS / 64];
    const int64_t n = a.n_reads;
    const int64_t per = (n + RL_SCAN_THREADS - 1) / RL_SCAN_THREADS;
    const int64_t k0 = min<int64_t>(n, threadIdx.x * per), k1 = min<int64_t>(n, k0 + per);
    int64_t s = 0, nre = 0, ndr = 0, nlim = 0, ntr = 0;
    for (int64_t k = k0; k < k1; k++) {
        s += a.cnt[k];
        nre += a.state[k] == ST_REALIGNED && a.bad[k] == BAD_NONE;
        ndr += a.state[k] == ST_DROPPED;
        nlim += a.bad[k] == BAD_LIMIT;
        ntr += a.bad[k] == BAD_TRACE;
    }
    int64_t total, tre, tdr, tlim, ttr;
    int64_t off = block_excl_sum<int64_t>(s, lds, &total);
    block_excl_sum<int64_t>(nre, lds, &tre);
    block_excl_sum<int64_t>(ndr, lds, &tdr);
    block_excl_sum<int64_t>(nlim, lds, &tlim);
    block_excl_sum<int64_t>(ntr, lds, &ttr);
    for (int64_t k = k0; k < k1; k++) {
        a.out_cigar_off[k] = off;
        off += a.cnt[k];
    }
    if (threadIdx.x == 0) {
        a.out_cigar_off[n] = total;
        a.counts[0] = total;
        a.counts[1] = tlim ? PV_ERR_LIMIT : ttr ? PV_ERR_STATE : total > a.cigar_cap ? PV_ERR_CAPACITY : PV_OK;
        a.counts[2] = tre;
        a.counts[3] = tdr;
    }
}

// one wavefront per read
__global__ __launch_bounds__(256) void k_rl_write(RlArgs a) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= a.n_reads) return;
    const int st = a.state[r];
    const int32_t* rs = a.res + r * 6;
    if (lane == 0) {
        a.out_state[r] = (uint8_t)st;
        a.out_score[r] = rs[0];
        for (int k = 0; k < 4; k++) a.out_ends[r * 4 + k] = st == ST_REALIGNED ? rs[1 + k] : 0;
        a.out_pos[r] = a.read_pos[r] + (st == ST_REALIGNED ? rs[1] : 0);
        if (a.out_band) a.out_band[r] = st == ST_REALIGNED ? rs[5] : 0;
    }
    if (a.counts[1] != PV_OK) return;
    const int64_t dst = a.out_cigar_off[r], n = a.cnt[r];
    const uint32_t* src = st == ST_REALIGNED ? a.tmp_cigar + 2 * (a.base_off[r] - a.base_off[0]) + 2 * r : a.cigar + a.cigar_off[r];
    for (int64_t k = lane; k < n; k += 64) a.out_cigar[dst + k] = src[k];
}

__global__ void k_rl_init(RlArgs a) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < a.n_reads) a.n_new[r] = -1;
}

}  // namespace

extern "C" int pv_polish_realign_dev(pv_ctx* ctx, const pv_batch_in* in, int64_t n_reads, int64_t n_bases, int64_t max_query_len,
                                     const int64_t* win_off, const uint8_t* win, pv_realign_out* out, int64_t* d_counts,
                                     void* stream) {
    PV_CHECK(ctx && in && out && d_counts && win_off, PV_ERR_INVALID, "null argument");
    PV_CHECK(in->n_regions >= 0 && n_reads >= 0 && n_bases >= 0 && max_query_len >= 0 && out->cigar_capacity >= 0,
             PV_ERR_INVALID, "negative sizes");
    PV_CHECK(n_reads < (1ll << 31), PV_ERR_LIMIT, "realign: too many reads for one launch");
    PV_CHECK(n_reads == 0 || (in->n_regions > 0 && in->ref_start && in->read_off && in->read_pos && in->base_off && in->bases &&
                              in->cigar_off && win && out->read_pos && out->cigar_off && out->score && out->ends && out->state),
             PV_ERR_INVALID, "realign: input or output arrays missing");
    PV_CHECK(out->cigar_off && (out->cigar_capacity == 0 || out->cigar), PV_ERR_INVALID, "realign: cigar output missing");
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = pv_pick_stream(ctx, stream);
    RlArgs a;
    memset(&a, 0, sizeof(a));
    a.n_regions = in->n_regions; a.n_reads = n_reads;
    a.ref_start = in->ref_start; a.read_off = in->read_off; a.read_pos = in->read_pos; a.base_off = in->base_off;
    a.bases = in->bases; a.cigar_off = in->cigar_off; a.cigar = in->cigar; a.win_off = win_off; a.win = win;
    a.out_pos = out->read_pos; a.out_cigar_off = out->cigar_off; a.out_cigar = out->cigar; a.cigar_cap = out->cigar_capacity;
    a.out_score = out->score; a.out_ends = out->ends; a.out_state = out->state; a.out_band = out->band; a.counts = d_counts;
    const size_t nr = (size_t)(n_reads > 0 ? n_reads : 1);
    int rc;
    if ((rc = pv_get(ctx, "rl.res", nr * 6, &a.res))) return rc;
    if ((rc = pv_get(ctx, "rl.state", nr, &a.state))) return rc;
    if ((rc = pv_get(ctx, "rl.bad", nr, &a.bad))) return rc;
    if ((rc = pv_get(ctx, "rl.n_new", nr, &a.n_new))) return rc;
    if ((rc = pv_get(ctx, "rl.cnt", nr, &a.cnt))) return rc;
    if ((rc = pv_get(ctx, "rl.tmp_cigar", (size_t)(2 * n_bases + 2 * n_reads + 1), &a.tmp_cigar))) return rc;
    a.pool_bytes = (int64_t)ctx->opt.realign_scratch_kb * 1024;
    if ((rc = pv_get(ctx, "rl.pool", (size_t)a.pool_bytes, &a.pool))) return rc;
    pv_prof_scope ps_all(ctx, "polish_realign", st);
    if (n_reads > 0) {
        const int64_t qmax = max_query_len > 0 ? max_query_len : 1;
        const int strip = (int)std::min<int64_t>(RL_MAX_STRIP, (qmax + 63) / 64);
        const unsigned nb = (unsigned)((n_reads + 255) / 256);
        k_rl_init<<<nb, 256, 0, st>>>(a);
        { pv_prof_scope ps(ctx, "k_rl_score_fwd", st);
          k_rl_score<false><<<(unsigned)n_reads, 64, (size_t)strip * 64 * 4, st>>>(a, strip); }
        { pv_prof_scope ps(ctx, "k_rl_score_rev", st);
          k_rl_score<true><<<(unsigned)n_reads, 64, (size_t)strip * 64 * 4, st>>>(a, strip); }
        // band rows: 3 x (window + 2) int16 of LDS; direction bytes from the pool in tiers of slot sizes (a full-size
        // region's read needs at most ~1.5 MB, so the first two tiers keep hundreds of workers busy)
        const size_t band_lds = (size_t)3 * (RL_MAX_WINDOW + 2) * sizeof(int16_t);
        { pv_prof_scope ps(ctx, "k_rl_bandw", st);
          k_rl_bandw<<<(unsigned)n_reads, RL_BAND_THREADS, band_lds, st>>>(a); }
        const int64_t slots[4] = {192 << 10, 1 << 20, 16 << 20, a.pool_bytes};
        static const char* names[4] = {"k_rl_band0", "k_rl_band1", "k_rl_band2", "k_rl_band3"};
        for (int t = 0; t < 4; t++) {
            const int64_t slot = std::min<int64_t>(slots[t], a.pool_bytes);
            const int64_t workers = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(a.pool_bytes / slot, 1 << 14), n_reads));
            pv_prof_scope ps(ctx, names[t], st);
            k_rl_band<<<(unsigned)workers, RL_BAND_THREADS, band_lds, st>>>(a, slot, t == 3);
        }
        k_rl_count<<<nb, 256, 0, st>>>(a);
    }
    { pv_prof_scope ps(ctx, "k_rl_scan", st); k_rl_scan<<<1, RL_SCAN_THREADS, 0, st>>>(a); }
    if (n_reads > 0) {
        pv_prof_scope ps(ctx, "k_rl_write", st);
        k_rl_write<<<(unsigned)((n_reads + 3) / 4), 256, 0, st>>>(a);
    }
    PV_HIP(hipGetLastError());
    return PV_OK;
}

template <typename T>
static int rl_stage(pv_ctx* ctx, const char* name, const T* src, size_t n, T** dst, hipStream_t st) {
    int rc = pv_get(ctx, name, n > 0 ? n : 1, dst);
    if (rc) return rc;
    if (n > 0) PV_HIP(hipMemcpyAsync(*dst, src, n * sizeof(T), hipMemcpyHostToDevice, st));
    return PV_OK;
}

extern "C" int pv_polish_realign(pv_ctx* ctx, const pv_batch_in* in, const int64_t* win_off, const uint8_t* win,
                                 pv_realign_out* out) {
    PV_CHECK(ctx && in && out && win_off, PV_ERR_INVALID, "null argument");
    PV_CHECK(in->n_regions >= 0 && out->cigar_capacity >= 0, PV_ERR_INVALID, "negative sizes");
    const int G = in->n_regions;
    PV_CHECK(G == 0 || (in->read_off && in->ref_start && in->base_off && in->cigar_off), PV_ERR_INVALID, "offset arrays missing");
    const int64_t n_reads = G ? in->read_off[G] - in->read_off[0] : 0;
    PV_CHECK(G == 0 || in->read_off[0] == 0, PV_ERR_INVALID, "read_off[0] must be 0");
    const int64_t n_bases = n_reads ? in->base_off[n_reads] : 0, n_cig = n_reads ? in->cigar_off[n_reads] : 0;
    PV_CHECK(n_reads == 0 || (in->base_off[0] == 0 && in->cigar_off[0] == 0), PV_ERR_INVALID, "base_off[0] and cigar_off[0] must be 0");
    int64_t qmax = 0;
    for (int64_t r = 0; r < n_reads; r++) {
        PV_CHECK(in->base_off[r + 1] >= in->base_off[r] && in->cigar_off[r + 1] >= in->cigar_off[r], PV_ERR_INVALID,
                 "offsets of read %lld decrease", (long long)r);
        qmax = std::max<int64_t>(qmax, in->base_off[r + 1] - in->base_off[r]);
    }
    for (int g = 0; g < G; g++)
        PV_CHECK(win_off[g + 1] >= win_off[g] && in->read_off[g + 1] >= in->read_off[g], PV_ERR_INVALID,
                 "offsets of region %d decrease", g);
    PV_CHECK(win_off[0] == 0, PV_ERR_INVALID, "win_off[0] must be 0");
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    pv_batch_in d;
    memset(&d, 0, sizeof(d));
    d.n_regions = G;
    const int64_t *d_woff = nullptr;
    const uint8_t* d_win = nullptr;
    int rc;
    if ((rc = rl_stage(ctx, "rls.ref_start", in->ref_start, (size_t)G, (int64_t**)&d.ref_start, st))) return rc;
    if ((rc = rl_stage(ctx, "rls.read_off", in->read_off, (size_t)G + 1, (int64_t**)&d.read_off, st))) return rc;
    if ((rc = rl_stage(ctx, "rls.read_pos", in->read_pos, (size_t)n_reads, (int64_t**)&d.read_pos, st))) return rc;
    if ((rc = rl_stage(ctx, "rls.base_off", in->base_off, (size_t)n_reads + 1, (int64_t**)&d.base_off, st))) return rc;
    if ((rc = rl_stage(ctx, "rls.bases", in->bases, (size_t)n_bases, (uint8_t**)&d.bases, st))) return rc;
    if ((rc = rl_stage(ctx, "rls.cigar_off", in->cigar_off, (size_t)n_reads + 1, (int64_t**)&d.cigar_off, st))) return rc;
    if ((rc = rl_stage(ctx, "rls.cigar", in->cigar, (size_t)n_cig, (uint32_t**)&d.cigar, st))) return rc;
    if ((rc = rl_stage(ctx, "rls.win_off", win_off, (size_t)G + 1, (int64_t**)&d_woff, st))) return rc;
    if ((rc = rl_stage(ctx, "rls.win", win, (size_t)(G ? win_off[G] : 0), (uint8_t**)&d_win, st))) return rc;
    pv_realign_out o;
    memset(&o, 0, sizeof(o));
    o.cigar_capacity = out->cigar_capacity;
    const size_t nr = (size_t)(n_reads > 0 ? n_reads : 1);
    int64_t* d_counts = nullptr;
    if ((rc = pv_get(ctx, "rls.read_pos_out", nr, &o.read_pos))) return rc;
    if ((rc = pv_get(ctx, "rls.cigar_off_out", nr + 1, &o.cigar_off))) return rc;
    if ((rc = pv_get(ctx, "rls.cigar_out", (size_t)(out->cigar_capacity > 0 ? out->cigar_capacity : 1), &o.cigar))) return rc;
    if ((rc = pv_get(ctx, "rls.score", nr, &o.score))) return rc;
    if ((rc = pv_get(ctx, "rls.ends", nr * 4, &o.ends))) return rc;
    if ((rc = pv_get(ctx, "rls.state", nr, &o.state))) return rc;
    if (out->band && (rc = pv_get(ctx, "rls.band", nr, &o.band))) return rc;
    if ((rc = pv_get(ctx, "rls.counts", (size_t)4, &d_counts))) return rc;
    rc = pv_polish_realign_dev(ctx, &d, n_reads, n_bases, qmax, d_woff, d_win, &o, d_counts, st);
    if (rc) return rc;
    int64_t counts[4];
    PV_HIP(hipMemcpyAsync(counts, d_counts, sizeof(counts), hipMemcpyDeviceToHost, st));
    PV_HIP(hipStreamSynchronize(st));
    out->n_cigar = counts[0];
    out->n_realigned = counts[2];
    out->n_dropped = counts[3];
    PV_CHECK(counts[1] != PV_ERR_LIMIT, PV_ERR_LIMIT,
             "realign: a read exceeds a limit (query > %d bases, window > %d bases, or its band does not fit the scratch pool "
             "of %d KB: option realign_scratch_kb)", RL_MAX_STRIP * 64, RL_MAX_WINDOW, ctx->opt.realign_scratch_kb);
    PV_CHECK(counts[1] != PV_ERR_STATE, PV_ERR_STATE, "realign: a traceback left its band");
    if (counts[1] == PV_ERR_CAPACITY) {
        pv_set_error("realign: cigar capacity too small: need %lld words", (long long)counts[0]);
        return PV_ERR_CAPACITY;
    }
    PV_CHECK(counts[1] == PV_OK, (int)counts[1], "realign: device status %lld", (long long)counts[1]);
    if (n_reads > 0) {
        PV_HIP(hipMemcpyAsync(out->read_pos, o.read_pos, (size_t)n_reads * 8, hipMemcpyDeviceToHost, st));
        PV_HIP(hipMemcpyAsync(out->cigar_off, o.cigar_off, ((size_t)n_reads + 1) * 8, hipMemcpyDeviceToHost, st));
        if (counts[0] > 0) PV_HIP(hipMemcpyAsync(out->cigar, o.cigar, (size_t)counts[0] * 4, hipMemcpyDeviceToHost, st));
        if (out->score) PV_HIP(hipMemcpyAsync(out->score, o.score, (size_t)n_reads * 4, hipMemcpyDeviceToHost, st));
        if (out->ends) PV_HIP(hipMemcpyAsync(out->ends, o.ends, (size_t)n_reads * 16, hipMemcpyDeviceToHost, st));
        if (out->state) PV_HIP(hipMemcpyAsync(out->state, o.state, (size_t)n_reads, hipMemcpyDeviceToHost, st));
        if (out->band) PV_HIP(hipMemcpyAsync(out->band, o.band, (size_t)n_reads * 4, hipMemcpyDeviceToHost, st));
        PV_HIP(hipStreamSynchronize(st));
    } else {
        out->cigar_off[0] = 0;
    }
    return PV_OK;
}
