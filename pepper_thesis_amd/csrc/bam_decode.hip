// bam_decode.hip — BAM record decode and region clipping on gfx950, from the bytes pv_bgzf_inflate_dev left in HBM to the
// builder's flat batch (pv_batch_in + read_hp). The specification is this repository's own reader, csrc/pv_io.cpp:
//   query_region  -> k_bam_walk   (the record walk of one interval: BAI chunks, Bgzf::tell's rule, tid / pos ends)
//   parse_record  -> k_bam_walk   (block_size range, negative l_seq, field sum) and k_bam_scan (CG:B,I long CIGAR)
//   aux_next / aux_hp -> aux_walk (one pass: first CG:B,I field, last HP field)
//   clip_append   -> clip_wave    (closed form of the CIGAR walk, see there)
//   fill_batch    -> k_bam_counts, the host step between the phases, k_bam_gather / k_bam_offsets / k_bam_fill
// Two phases, because the host sizes the outputs (and decides down-sampling) from the per-interval counts:
//   scan: k_bam_walk (one wave per interval; a chain of dependent loads) lists the records of the interval;
//         k_bam_base (one block) turns the per-interval record numbers into a compact numbering;
//         k_bam_scan (one wave per record) filters, clips and measures every record;
//         k_bam_counts (one block per interval) numbers the kept reads and sums reads / bases / CIGAR words.
//   fill: k_bam_gather (one thread per output read) names the record behind every output read (reservoir order where the
//         host sent indices); k_bam_offsets (one block) is the exclusive scan that gives base_off / cigar_off;
//         k_bam_fill (one wave per output read) unpacks SEQ, copies QUAL, re-packs the clipped CIGAR.
// No global atomics: every count comes from a scan or a reduction. No workspace of the context is used (the caller owns
// `ws`), so the calls run on a stream of their own beside the builder and the RNN.
//
// Safety by construction. The inflated bytes of the blocks of a reader group lie end to end in `data` in file order, so the
// uncompressed stream is contiguous in `data` exactly where next_coffset[i] == coffset[i + 1]. k_bam_walk accepts a record only
// when every block under [record, record + block_size) is chained that way, inflated without error, and inside
// [0, data_bytes); it has then also checked 32 + l_read_name + 4 n_cigar + (l_seq + 1) / 2 + l_seq <= block_size. Every later
// load is at an offset below block_size of a record accepted there (the aux walk carries its own end), every store is bounded
// by the capacity its array was sized with, and every loop advances by at least one byte, CIGAR word or block per turn.
#include "pv_common.hpp"

namespace {

constexpr int WV = 64;

__device__ __forceinline__ uint32_t ld16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
__device__ __forceinline__ uint32_t ld32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// the caller's workspace, carved: S record slots (interval i owns slots [iv_rec_off[i], iv_rec_off[i + 1])), N intervals
struct Ws {
    int64_t* rec_p;      // [S] offset in `data` of the record body (the byte after block_size)
    int64_t* rec_pos0;   // [S] first kept reference position
    int64_t* rec_cig;    // [S] offset in `data` of the CIGAR words in use (the record's, or the CG tag's)
    int32_t* rec_bs;     // [S] block_size
    int32_t* rec_err;    // [S] PV_BAMDEC_* of the record (0 = none)
    int32_t* rec_nb;     // [S] kept bases (0 = read not kept)
    int32_t* rec_nc;     // [S] kept CIGAR words
    int32_t* rec_q0;     // [S] first kept SEQ index
    int32_t* rec_ncig;   // [S] CIGAR words in use
    int32_t* rec_hp;     // [S] HP tag
    int32_t* kept;       // [S] kept[slot0 + k] = index (inside the interval) of the interval's k-th kept read
    int32_t* src;        // [S] slot behind output read j (-1: bad index)
    int64_t* iv_werr;    // [N][3] walker: offset in `data` of the offender, two details
    int64_t* rec_base;   // [N+1] exclusive scan of iv_nrec
    int32_t* iv_nrec;    // [N] records listed
    int32_t* iv_wstatus; // [N] walker status
    int32_t* iv_nkept;   // [N] reads kept
};

__host__ __device__ inline int64_t up8(int64_t v) { return (v + 7) & ~(int64_t)7; }

__host__ __device__ inline int64_t ws_carve(uint8_t* base, int64_t N, int64_t S, Ws* w) {
    int64_t o = 0;
    const int64_t s8 = up8(8 * S), s4 = up8(4 * S);
#define PV_TAKE(field, type, bytes) do { if (w) w->field = (type*)(base + o); o += (bytes); } while (0)
    PV_TAKE(rec_p, int64_t, s8); PV_TAKE(rec_pos0, int64_t, s8); PV_TAKE(rec_cig, int64_t, s8);
    PV_TAKE(rec_bs, int32_t, s4); PV_TAKE(rec_err, int32_t, s4); PV_TAKE(rec_nb, int32_t, s4); PV_TAKE(rec_nc, int32_t, s4);
    PV_TAKE(rec_q0, int32_t, s4); PV_TAKE(rec_ncig, int32_t, s4); PV_TAKE(rec_hp, int32_t, s4); PV_TAKE(kept, int32_t, s4);
    PV_TAKE(src, int32_t, s4);
    PV_TAKE(iv_werr, int64_t, 24 * N); PV_TAKE(rec_base, int64_t, 8 * (N + 1));
    PV_TAKE(iv_nrec, int32_t, up8(4 * N)); PV_TAKE(iv_wstatus, int32_t, up8(4 * N)); PV_TAKE(iv_nkept, int32_t, up8(4 * N));
#undef PV_TAKE
    return o + 8;
}

// ---- record walk ----------------------------------------------------------------------------------------------------
// first block index in [lo, hi) whose coffset is >= co
__device__ inline int64_t blk_lower_bound(const int64_t* coffset, int64_t lo, int64_t hi, int64_t co) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (coffset[mid] < co) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ inline int blk_check(const pv_bam_decode_in& a, int64_t b) {
    const int64_t o = a.out_off[b], n = a.isize[b];
    if (o < 0 || n < 0 || n > 65536 || o + n > a.data_bytes) return PV_BAMDEC_BAD_TABLE;
    if (a.blk_status[b] != 0) return PV_BAMDEC_BAD_BLOCK;
    return PV_BAMDEC_OK;
}

// Move the block cursor so that `target` (an offset in `data`, at or after the cursor's block start) lies in or at the end of
// block b: the reader's load_block(next_coffset) for every block a read runs through. One block per turn.
__device__ inline int blk_advance(const pv_bam_decode_in& a, int64_t b1, int64_t& b, int64_t target, int64_t& bad_block) {
    while (target > a.out_off[b] + a.isize[b]) {
        if (b + 1 >= b1 || a.coffset[b + 1] != a.next_coffset[b]) return PV_BAMDEC_PAST_PLAN;
        if (a.out_off[b + 1] != a.out_off[b] + a.isize[b]) return PV_BAMDEC_BAD_TABLE;
        b++;
        const int rc = blk_check(a, b);
        if (rc) { bad_block = b; return rc; }
    }
    return PV_BAMDEC_OK;
}

// One wave per interval; the walk is scalar by nature (every record's place comes from the one before), so all lanes run
// the same chain on the same addresses and lane 0 stores.
__global__ __launch_bounds__(WV) void k_bam_walk(pv_bam_decode_in a, Ws w) {
    const int iv = blockIdx.x;
    if (iv >= a.n_intervals) return;
    const int64_t b0 = a.iv_blk0[iv], b1 = a.iv_blk1[iv];
    const int32_t tid = a.iv_tid[iv];
    const int64_t qend = a.iv_re[iv];
    const int64_t slot0 = a.iv_rec_off[iv], cap = a.iv_rec_off[iv + 1] - slot0;
    const bool writer = threadIdx.x == 0;
    int64_t n = 0, err_at = -1, d1 = 0, d2 = 0;
    int status = PV_BAMDEC_OK;
    bool done = false;
    if (b0 < 0 || b1 > a.n_blocks || b0 > b1 || slot0 < 0 || cap < 0 || slot0 + cap > a.rec_slots) status = PV_BAMDEC_BAD_TABLE;
    if (a.iv_chunk_off[iv] < 0 || a.iv_chunk_off[iv] > a.iv_chunk_off[iv + 1] || a.iv_chunk_off[iv + 1] > a.n_chunks) status = PV_BAMDEC_BAD_TABLE;
    for (int64_t ci = a.iv_chunk_off[iv]; ci < a.iv_chunk_off[iv + 1] && !done && status == PV_BAMDEC_OK; ci++) {
        const uint64_t cbeg = (uint64_t)a.chunk_beg[ci], cend = (uint64_t)a.chunk_end[ci];
        // Bgzf::seek
        const int64_t co = (int64_t)(cbeg >> 16);
        int64_t b = blk_lower_bound(a.coffset, b0, b1, co);
        if (b >= b1 || a.coffset[b] != co) { status = PV_BAMDEC_PAST_PLAN; d1 = co; break; }
        if ((status = blk_check(a, b)) != 0) { d1 = b; break; }
        if ((int64_t)(cbeg & 0xFFFF) > a.isize[b]) { status = PV_BAMDEC_SEEK; d1 = co; break; }
        int64_t p = a.out_off[b] + (int64_t)(cbeg & 0xFFFF);
        for (;;) {
            // Bgzf::tell: a block consumed to its end reports offset 0 of the next one
            const int64_t bend = a.out_off[b] + a.isize[b];
            const uint64_t tell = (a.isize[b] > 0 && p >= bend) ? ((uint64_t)a.next_coffset[b] << 16)
                                                                : (((uint64_t)a.coffset[b] << 16) | (uint64_t)((p - a.out_off[b]) & 0xFFFF));
            if (tell >= cend) break;
            err_at = p;
            if ((status = blk_advance(a, b1, b, p + 4, d1)) != 0) break;
            const uint32_t bs = ld32(a.data + p);
            if (bs < 32 || bs > (1u << 30)) { status = PV_BAMDEC_BLOCK_SIZE; d1 = bs; break; }
            p += 4;
            if ((status = blk_advance(a, b1, b, p + (int64_t)bs, d1)) != 0) break;
            const uint8_t* r = a.data + p;   // [r, r + bs) is chained, inflated and inside `data`
            const int32_t rtid = (int32_t)ld32(r);
            const int64_t rpos = (int32_t)ld32(r + 4);
            const int64_t l_name = r[8], n_cig = ld16(r + 12), l_seq = (int32_t)ld32(r + 16);
            if (l_seq < 0) { status = PV_BAMDEC_BAD_RECORD; d1 = bs; d2 = -1; break; }
            const int64_t need = 32 + l_name + 4 * n_cig + (l_seq + 1) / 2 + l_seq;
            if (need > (int64_t)bs) { status = PV_BAMDEC_BAD_RECORD; d1 = bs; d2 = need; break; }
            if (rtid != tid) {
                if (rtid > tid) { done = true; break; }
            } else {
                if (rpos >= qend) { done = true; break; }
                if (n >= cap) { status = PV_BAMDEC_BAD_TABLE; break; }
                if (writer) { w.rec_p[slot0 + n] = p; w.rec_bs[slot0 + n] = (int32_t)bs; }
                n++;
            }
            p += (int64_t)bs;   // at least 36 bytes per turn
        }
    }
    // chunks past the linear-index bound were left out of the plan: only a walk that met its end before them is complete
    if (status == PV_BAMDEC_OK) err_at = -1;   // (err_at followed the walk: no offender, no offset)
    if (!done && status == PV_BAMDEC_OK && a.iv_dropped[iv]) status = PV_BAMDEC_PAST_PLAN;
    if (writer) {
        w.iv_nrec[iv] = (int32_t)n;
        w.iv_wstatus[iv] = status;
        w.iv_werr[3 * iv] = err_at; w.iv_werr[3 * iv + 1] = d1; w.iv_werr[3 * iv + 2] = d2;
    }
}

// exclusive scan of the per-interval record numbers (N is a few hundred at most): one block
__global__ __launch_bounds__(256) void k_bam_base(int32_t n_intervals, Ws w) {
    __shared__ int64_t s[256];
    int64_t carry = 0;
    for (int32_t i0 = 0; i0 < n_intervals; i0 += 256) {
        const int32_t i = i0 + (int32_t)threadIdx.x;
        const int64_t v = i < n_intervals ? w.iv_nrec[i] : 0;
        s[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const int64_t t = (int)threadIdx.x >= d ? s[threadIdx.x - d] : 0;
            __syncthreads();
            s[threadIdx.x] += t;
            __syncthreads();
        }
        if (i < n_intervals) w.rec_base[i] = carry + s[threadIdx.x] - v;
        carry += s[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) w.rec_base[n_intervals] = carry;
}

// ---- per record ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t wave_incl_scan(int64_t v, int lane) {
    for (int d = 1; d < WV; d <<= 1) {
        const int64_t t = __shfl_up((long long)v, d, WV);
        if (lane >= d) v += t;
    }
    return v;
}
__device__ __forceinline__ int64_t wave_max(int64_t v) {
    for (int d = WV / 2; d > 0; d >>= 1) {
        const int64_t t = __shfl_xor((long long)v, d, WV);
        v = t > v ? t : v;
    }
    return v;
}

struct Clip {
    int64_t pos_start, q_first, q_end;
    int32_t n_words;
    bool found, err;
};

// clip_append for one wave: the CIGAR walk in closed form, 64 operations per turn.
// Until the walk ends, the reader's cur_pos before operation k is P_k = pos + (reference lengths of the operations before k)
// and cur_idx is Q_k = (query lengths before k): an operation cut at `stop` leaves cur_pos = stop + 1, the next turn breaks, and
// P_{k+1} > stop says the same. So the walked operations are the prefix with P_k <= stop, and with f = the first M/=/X
// operation that keeps a base:
//   M/=/X  i0 = min(start - P, len) if P < start else 0; kept = max(0, min(len - i0, stop - (P + i0) + 1))
//   I/S    kept = len when start <= P <= stop and k > f
//   D/N    kept = min(len, stop - P + 1) under the same condition
//   H, P, B and unknown codes: nothing.
// pos = P_f + i0_f, the kept SEQ range starts at Q_f + i0_f and ends with the last kept M/=/X/I/S operation; a kept M/=/X/I/S
// operation that ends past l_seq is the reader's "CIGAR longer than SEQ". WRITE: the kept words go to out[0 .. out_cap).
template <bool WRITE>
__device__ Clip clip_wave(const uint8_t* cig, int64_t n_ops, int64_t pos, int64_t l_seq, int64_t start, int64_t stop, uint32_t* out,
                          int64_t out_cap) {
    const int lane = threadIdx.x & (WV - 1);
    const uint64_t lt = lane ? (~0ull >> (WV - lane)) : 0ull;
    Clip c;
    c.pos_start = -1; c.q_first = 0; c.q_end = 0; c.n_words = 0; c.found = false; c.err = false;
    int64_t Pc = pos, Qc = 0;
    for (int64_t k0 = 0; k0 < n_ops && Pc <= stop; k0 += WV) {
        const int64_t k = k0 + lane;
        const bool in = k < n_ops;
        const uint32_t word = in ? ld32(cig + 4 * k) : 0u;
        const int op = (int)(word & 0xF);
        const int64_t len = word >> 4;
        const bool isM = op == 0 || op == 7 || op == 8, isIS = op == 1 || op == 4, isDN = op == 2 || op == 3;
        const int64_t r = (in && (isM || isDN)) ? len : 0, q = (in && (isM || isIS)) ? len : 0;
        const int64_t ri = wave_incl_scan(r, lane), qi = wave_incl_scan(q, lane);
        const int64_t P = Pc + ri - r, Q = Qc + qi - q;
        const bool active = in && P <= stop;
        int64_t i0 = 0, nM = 0;
        if (active && isM) {
            if (P < start) i0 = (start - P) < len ? (start - P) : len;
            const int64_t room = stop - (P + i0) + 1;
            nM = (len - i0) < room ? (len - i0) : room;
            if (nM < 0) nM = 0;
        }
        const bool hit = nM > 0;
        const uint64_t hits = __ballot(hit);
        if (!c.found && hits) {
            const int fl = __ffsll((unsigned long long)hits) - 1;
            c.pos_start = __shfl((long long)(P + i0), fl, WV);
            c.q_first = __shfl((long long)(Q + i0), fl, WV);
        }
        const bool after_f = c.found || (hits & lt) != 0;
        const bool cond = active && P >= start && after_f;
        int64_t kept = 0, qe = 0;
        bool bad = false;
        if (hit) { kept = nM; qe = Q + i0 + nM; bad = qe > l_seq; }
        else if (isIS && cond) { kept = len; qe = Q + len; bad = qe > l_seq; }
        else if (isDN && cond) { const int64_t room = stop - P + 1; kept = len < room ? len : room; }
        const uint64_t emits = __ballot(kept > 0);
        if (WRITE && kept > 0) {
            const int64_t at = c.n_words + __popcll(emits & lt);
            if (at < out_cap) out[at] = (uint32_t)((kept << 4) | (uint32_t)op);
        }
        c.n_words += __popcll(emits);
        if (__ballot(bad)) c.err = true;
        const int64_t m = wave_max(qe);
        if (m > c.q_end) c.q_end = m;
        if (hits) c.found = true;
        Pc += __shfl((long long)ri, WV - 1, WV);
        Qc += __shfl((long long)qi, WV - 1, WV);
    }
    return c;
}

// aux_next over the whole aux area [s, end) of record r (offsets from r), wave-uniform: the first CG:B,I field (offset of its
// words and their number) and the last HP field of an integer type. Stops at the first field that does not fit, as the reader
// does. Every turn consumes at least three bytes.
__device__ void aux_walk(const uint8_t* r, int64_t s, int64_t end, int64_t& cg_at, int64_t& cg_n, int32_t& hp) {
    const int lane = threadIdx.x & (WV - 1);
    cg_at = -1; cg_n = 0; hp = 0;
    while (s < end) {
        if (end - s < 3) return;
        const uint8_t t0 = r[s], t1 = r[s + 1], ty = r[s + 2];
        s += 3;
        int64_t vb;
        switch (ty) {
            case 'A': case 'c': case 'C': vb = 1; break;
            case 's': case 'S': vb = 2; break;
            case 'i': case 'I': case 'f': vb = 4; break;
            case 'Z': case 'H': {
                int64_t at = -1;
                for (int64_t e = s; e < end && at < 0; e += WV) {   // 64 bytes per turn
                    const uint64_t z = __ballot(e + lane < end && r[e + lane] == 0);
                    if (z) at = e + __ffsll((unsigned long long)z) - 1;
                }
                if (at < 0) return;
                vb = at - s + 1;
                break;
            }
            case 'B': {
                if (end - s < 5) return;
                const uint8_t st = r[s];
                const int64_t ne = ld32(r + s + 1);
                const int es = (st == 'c' || st == 'C') ? 1 : (st == 's' || st == 'S') ? 2 : (st == 'i' || st == 'I' || st == 'f') ? 4 : 0;
                if (!es) return;
                vb = 5 + ne * es;
                break;
            }
            default: return;
        }
        if (end - s < vb) return;
        if (t0 == 'H' && t1 == 'P') {
            switch (ty) {
                case 'c': hp = (int8_t)r[s]; break;
                case 'C': hp = r[s]; break;
                case 's': hp = (int16_t)ld16(r + s); break;
                case 'S': hp = (int32_t)ld16(r + s); break;
                case 'i': case 'I': hp = (int32_t)ld32(r + s); break;
                default: break;
            }
        }
        if (cg_at < 0 && t0 == 'C' && t1 == 'G' && ty == 'B' && r[s] == 'I') { cg_at = s + 5; cg_n = ld32(r + s + 1); }
        s += vb;
    }
}

// interval of compact record number x: the last i with rec_base[i] <= x
__device__ inline int32_t find_interval(const int64_t* base, int32_t n, int64_t x) {
    int32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (base[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// One wave per record. The reader's overlap test (bam_endpos > start) needs no pass of its own: a record that ends at or
// before the window keeps no base in the clip (every M/=/X operation lies left of `start`), raises no "CIGAR longer than SEQ"
// (that needs a kept operation) and is dropped as "nothing kept"; pos < end holds for every listed record.
__global__ __launch_bounds__(256) void k_bam_scan(pv_bam_decode_in a, Ws w) {
    const int lane = threadIdx.x & (WV - 1);
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x / WV) + (threadIdx.x / WV);
    const int64_t n_waves = (int64_t)gridDim.x * (blockDim.x / WV);
    const int64_t total = w.rec_base[a.n_intervals];
    for (int64_t x = wave; x < total; x += n_waves) {
        const int32_t iv = find_interval(w.rec_base, a.n_intervals, x);
        const int64_t slot = a.iv_rec_off[iv] + (x - w.rec_base[iv]);
        const uint8_t* r = a.data + w.rec_p[slot];
        const int64_t bs = w.rec_bs[slot];
        const int64_t pos = (int32_t)ld32(r + 4);
        const int64_t l_name = r[8], n_cig = ld16(r + 12), l_seq = (int32_t)ld32(r + 16);
        const int mapq = r[9];
        const uint32_t flag = ld16(r + 14);
        int32_t nb = 0, nc = 0, q0 = 0, hp = 0, err = 0, ncig_used = 0;
        int64_t pos0 = 0, cig_at = 32 + l_name;
        const bool pass = !(flag & (0x200 | 0x400 | 0x100 | 0x4)) && (a.include_supplementary || !(flag & 0x800)) && mapq >= a.min_mapq;
        if (pass) {
            int64_t cg_at, cg_n, n_ops = n_cig;
            aux_walk(r, 32 + l_name + 4 * n_cig + (l_seq + 1) / 2 + l_seq, bs, cg_at, cg_n, hp);
            if (n_cig >= 1 && (int32_t)ld32(r) >= 0 && pos >= 0 && cg_at >= 0) {   // the <l_seq>S<rlen>N placeholder of a long CIGAR
                const uint32_t c0 = ld32(r + cig_at);
                if ((c0 & 0xF) == 4 && (int64_t)(c0 >> 4) == l_seq) { cig_at = cg_at; n_ops = cg_n; }
            }
            const Clip c = clip_wave<false>(r + cig_at, n_ops, pos, l_seq, a.iv_rs[iv], a.iv_re[iv], nullptr, 0);
            if (c.err) err = PV_BAMDEC_CIGAR_LONGER;
            else if (c.found) {
                nb = (int32_t)(c.q_end - c.q_first); nc = c.n_words; q0 = (int32_t)c.q_first; pos0 = c.pos_start;
                ncig_used = (int32_t)n_ops;
            }
        }
        if (lane == 0) {
            w.rec_err[slot] = err; w.rec_nb[slot] = nb; w.rec_nc[slot] = nc; w.rec_q0[slot] = q0; w.rec_hp[slot] = hp;
            w.rec_pos0[slot] = pos0; w.rec_cig[slot] = w.rec_p[slot] + cig_at; w.rec_ncig[slot] = ncig_used;
        }
    }
}

// virtual offset (coffset << 16 | offset in the block) of offset `at` of `data`: the last block that starts at or before it
__device__ inline int64_t voffset_of(const pv_bam_decode_in& a, int64_t at) {
    if (at < 0 || a.n_blocks <= 0) return -1;
    int64_t lo = 0, hi = a.n_blocks;
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a.out_off[mid] <= at) lo = mid; else hi = mid;
    }
    return (a.coffset[lo] << 16) | ((at - a.out_off[lo]) & 0xFFFF);
}

// One block per interval: kept reads numbered in record order (kept[]), their sums, and the first offender in walk order
// (a record's own error comes before the walker's, which stopped after the last listed record).
// counts[iv] = {reads kept, bases, CIGAR words, status, virtual offset of the offender (-1 none), detail, detail, records}
__global__ __launch_bounds__(256) void k_bam_counts(pv_bam_decode_in a, Ws w, int64_t* counts) {
    __shared__ int64_t s_n[256], s_b[256], s_c[256], s_e[256];
    const int iv = blockIdx.x;
    const int t = threadIdx.x;
    const int64_t slot0 = a.iv_rec_off[iv];
    const int32_t n = w.iv_nrec[iv];
    int64_t carry = 0, bases = 0, words = 0, first_err = INT64_MAX;
    for (int32_t i0 = 0; i0 < n; i0 += 256) {
        const int32_t i = i0 + t;
        const bool in = i < n;
        const int32_t nb = in ? w.rec_nb[slot0 + i] : 0;
        const int64_t keep = nb > 0 ? 1 : 0;
        if (in && w.rec_err[slot0 + i] != 0 && (int64_t)i < first_err) first_err = i;
        bases += nb;
        words += in ? w.rec_nc[slot0 + i] : 0;
        s_n[t] = keep;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const int64_t v = t >= d ? s_n[t - d] : 0;
            __syncthreads();
            s_n[t] += v;
            __syncthreads();
        }
        if (keep) w.kept[slot0 + carry + s_n[t] - 1] = i;
        carry += s_n[255];
        __syncthreads();
    }
    s_b[t] = bases; s_c[t] = words; s_e[t] = first_err;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (t < d) {
            s_b[t] += s_b[t + d]; s_c[t] += s_c[t + d];
            s_e[t] = s_e[t + d] < s_e[t] ? s_e[t + d] : s_e[t];
        }
        __syncthreads();
    }
    if (t == 0) {
        int64_t* c = counts + 8 * (int64_t)iv;
        int64_t status = w.iv_wstatus[iv], at = w.iv_werr[3 * iv], d1 = w.iv_werr[3 * iv + 1], d2 = w.iv_werr[3 * iv + 2];
        if (s_e[0] != INT64_MAX) {
            status = w.rec_err[slot0 + s_e[0]];
            at = w.rec_p[slot0 + s_e[0]] - 4; d1 = w.rec_bs[slot0 + s_e[0]]; d2 = 0;
        }
        w.iv_nkept[iv] = (int32_t)carry;
        c[0] = carry; c[1] = s_b[0]; c[2] = s_c[0]; c[3] = status; c[4] = voffset_of(a, at); c[5] = d1; c[6] = d2; c[7] = n;
    }
}

// ---- fill --------------------------------------------------------------------------------------------------------------
struct FillArgs {
    int32_t n_regions;
    const int32_t* reg_iv;     // [n_regions] interval of every output region
    const int64_t* read_off;   // [n_regions+1]
    const int64_t* sel_off;    // [n_regions] -1: every kept read in record order; else the region's indices start at sel[sel_off]
    const int64_t* sel;
    int64_t n_sel, n_reads, base_cap, cigar_cap;
    int64_t *read_pos, *base_off, *cigar_off;
    uint8_t *read_flags, *read_mapq, *bases, *quals;
    uint32_t* cigar;
    int32_t* read_hp;
    int64_t* totals;           // {reads, bases, CIGAR words, status}
};

__global__ __launch_bounds__(256) void k_bam_gather(pv_bam_decode_in a, Ws w, FillArgs f) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= f.n_reads) return;
    int32_t lo = 0, hi = f.n_regions;
    while (hi - lo > 1) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (f.read_off[mid] <= j) lo = mid; else hi = mid;
    }
    int32_t slot = -1;
    const int32_t iv = f.reg_iv[lo];
    if (iv >= 0 && iv < a.n_intervals) {
        int64_t k = j - f.read_off[lo];
        const int64_t so = f.sel_off[lo];
        if (so >= 0) k = (so + k < f.n_sel) ? f.sel[so + k] : -1;
        if (k >= 0 && k < w.iv_nkept[iv]) {
            const int64_t slot0 = a.iv_rec_off[iv];
            slot = (int32_t)(slot0 + w.kept[slot0 + k]);
        }
    }
    w.src[j] = slot;
}

// exclusive scans of the output reads' kept bases and CIGAR words: one block, 1024 reads per turn
__global__ __launch_bounds__(1024) void k_bam_offsets(Ws w, FillArgs f) {
    __shared__ int64_t s_b[1024], s_c[1024];
    __shared__ int s_bad;
    const int t = threadIdx.x;
    if (t == 0) s_bad = 0;
    __syncthreads();
    int64_t cb = 0, cc = 0;
    for (int64_t j0 = 0; j0 < f.n_reads; j0 += 1024) {
        const int64_t j = j0 + t;
        int64_t nb = 0, nc = 0;
        if (j < f.n_reads) {
            const int32_t slot = w.src[j];
            if (slot >= 0) { nb = w.rec_nb[slot]; nc = w.rec_nc[slot]; }
            else s_bad = 1;
        }
        s_b[t] = nb; s_c[t] = nc;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const int64_t vb = t >= d ? s_b[t - d] : 0, vc = t >= d ? s_c[t - d] : 0;
            __syncthreads();
            s_b[t] += vb; s_c[t] += vc;
            __syncthreads();
        }
        if (j < f.n_reads) { f.base_off[j] = cb + s_b[t] - nb; f.cigar_off[j] = cc + s_c[t] - nc; }
        cb += s_b[1023]; cc += s_c[1023];
        __syncthreads();
    }
    if (t == 0) {
        f.base_off[f.n_reads] = cb; f.cigar_off[f.n_reads] = cc;
        f.totals[0] = f.n_reads; f.totals[1] = cb; f.totals[2] = cc;
        f.totals[3] = s_bad ? PV_ERR_INVALID : (cb > f.base_cap || cc > f.cigar_cap) ? PV_ERR_CAPACITY : PV_OK;
    }
}

__constant__ uint8_t c_nt16[16] = {'=', 'A', 'C', 'M', 'G', 'R', 'S', 'V', 'T', 'W', 'Y', 'H', 'K', 'D', 'B', 'N'};

// One wave per output read: 4-bit SEQ -> letters, QUAL, the clipped CIGAR words, the per-read fields.
__global__ __launch_bounds__(256) void k_bam_fill(pv_bam_decode_in a, Ws w, FillArgs f) {
    const int lane = threadIdx.x & (WV - 1);
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x / WV) + (threadIdx.x / WV);
    const int64_t n_waves = (int64_t)gridDim.x * (blockDim.x / WV);
    for (int64_t j = wave; j < f.n_reads; j += n_waves) {
        const int32_t slot = w.src[j];
        if (slot < 0) continue;
        const int64_t bo = f.base_off[j], co = f.cigar_off[j];
        const int64_t nb = w.rec_nb[slot], nc = w.rec_nc[slot];
        if (bo + nb > f.base_cap || co + nc > f.cigar_cap) continue;   // (k_bam_offsets reported PV_ERR_CAPACITY)
        const uint8_t* r = a.data + w.rec_p[slot];
        const int64_t l_name = r[8], n_cig = ld16(r + 12), l_seq = (int32_t)ld32(r + 16);
        const uint8_t* seq = r + 32 + l_name + 4 * n_cig;
        const uint8_t* qual = seq + (l_seq + 1) / 2;
        const int64_t q0 = w.rec_q0[slot];
        for (int64_t i = lane; i < nb; i += WV) {   // q0 + nb <= l_seq (k_bam_scan)
            const int64_t q = q0 + i;
            const uint8_t two = seq[q >> 1];
            f.bases[bo + i] = c_nt16[(q & 1) ? (two & 0xF) : (two >> 4)];
            f.quals[bo + i] = qual[q];
        }
        // the interval's window: the region's interval is the one the record was listed for
        int32_t lo = 0, hi = f.n_regions;
        while (hi - lo > 1) {
            const int32_t mid = lo + ((hi - lo) >> 1);
            if (f.read_off[mid] <= j) lo = mid; else hi = mid;
        }
        const int32_t iv = f.reg_iv[lo];
        clip_wave<true>(a.data + w.rec_cig[slot], w.rec_ncig[slot], (int32_t)ld32(r + 4), l_seq, a.iv_rs[iv], a.iv_re[iv], f.cigar + co, nc);
        if (lane == 0) {
            f.read_pos[j] = w.rec_pos0[slot];
            f.read_flags[j] = (ld16(r + 14) & 0x10) ? 1 : 0;
            f.read_mapq[j] = r[9];
            f.read_hp[j] = w.rec_hp[slot];
        }
    }
}

int check_in(pv_ctx* ctx, const pv_bam_decode_in* in, void* ws, int64_t ws_bytes) {
    PV_CHECK(ctx && in && ws, PV_ERR_INVALID, "null argument");
    PV_CHECK(in->n_intervals >= 0 && in->n_blocks >= 0 && in->data_bytes >= 0 && in->rec_slots >= 0 && in->n_chunks >= 0, PV_ERR_INVALID, "negative sizes");
    PV_CHECK(in->n_chunks == 0 || (in->chunk_beg && in->chunk_end), PV_ERR_INVALID, "bam_decode: chunk table missing");
    PV_CHECK(in->rec_slots < (1ll << 31), PV_ERR_LIMIT, "bam_decode: too many record slots for one launch");
    PV_CHECK(in->n_intervals == 0 || (in->iv_tid && in->iv_rs && in->iv_re && in->iv_blk0 && in->iv_blk1 && in->iv_chunk_off && in->iv_dropped && in->iv_rec_off),
             PV_ERR_INVALID, "bam_decode: interval table missing");
    PV_CHECK(in->n_blocks == 0 || (in->data && in->coffset && in->next_coffset && in->isize && in->out_off && in->blk_status), PV_ERR_INVALID,
             "bam_decode: block table missing");
    PV_CHECK(ws_bytes >= ws_carve(nullptr, in->n_intervals, in->rec_slots, nullptr), PV_ERR_CAPACITY, "bam_decode: workspace too small");
    PV_CHECK(((uintptr_t)ws & 7) == 0, PV_ERR_INVALID, "bam_decode: workspace not 8-byte aligned");
    return PV_OK;
}

}  // namespace

extern "C" int64_t pv_bam_decode_ws_bytes(int64_t n_intervals, int64_t rec_slots) {
    if (n_intervals < 0 || rec_slots < 0) return -1;
    return ws_carve(nullptr, n_intervals, rec_slots, nullptr);
}

extern "C" int pv_bam_scan_dev(pv_ctx* ctx, const pv_bam_decode_in* in, void* ws, int64_t ws_bytes, int64_t* d_iv_counts, void* stream) {
    int rc = check_in(ctx, in, ws, ws_bytes);
    if (rc) return rc;
    PV_CHECK(d_iv_counts || in->n_intervals == 0, PV_ERR_INVALID, "null argument");
    if (in->n_intervals == 0) return PV_OK;
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = pv_pick_stream(ctx, stream);
    Ws w;
    ws_carve((uint8_t*)ws, in->n_intervals, in->rec_slots, &w);
    k_bam_walk<<<(unsigned)in->n_intervals, WV, 0, st>>>(*in, w);
    k_bam_base<<<1, 256, 0, st>>>(in->n_intervals, w);
    const int64_t waves = in->rec_slots < 16384 ? (in->rec_slots > 0 ? in->rec_slots : 1) : 16384;
    k_bam_scan<<<(unsigned)((waves + 3) / 4), 256, 0, st>>>(*in, w);
    k_bam_counts<<<(unsigned)in->n_intervals, 256, 0, st>>>(*in, w, d_iv_counts);
    PV_HIP(hipGetLastError());
    return PV_OK;
}

extern "C" int pv_bam_fill_dev(pv_ctx* ctx, const pv_bam_decode_in* in, void* ws, int64_t ws_bytes, int32_t n_regions,
                               const int32_t* reg_iv, const int64_t* read_off, const int64_t* sel_off, const int64_t* sel,
                               int64_t n_sel, int64_t n_reads, int64_t base_capacity, int64_t cigar_capacity, const pv_batch_in* out,
                               int32_t* read_hp, int64_t* d_totals, void* stream) {
    int rc = check_in(ctx, in, ws, ws_bytes);
    if (rc) return rc;
    PV_CHECK(out && d_totals && n_regions > 0 && reg_iv && read_off && sel_off, PV_ERR_INVALID, "bam_fill: region table missing");
    PV_CHECK(n_reads > 0 && n_reads <= in->rec_slots && n_sel >= 0 && base_capacity >= 0 && cigar_capacity >= 0 && (n_sel == 0 || sel),
             PV_ERR_INVALID, "bam_fill: bad sizes");
    PV_CHECK(out->read_pos && out->read_flags && out->read_mapq && out->base_off && out->bases && out->quals && out->cigar_off && out->cigar && read_hp,
             PV_ERR_INVALID, "bam_fill: output arrays missing");
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = pv_pick_stream(ctx, stream);
    Ws w;
    ws_carve((uint8_t*)ws, in->n_intervals, in->rec_slots, &w);
    FillArgs f;
    f.n_regions = n_regions; f.reg_iv = reg_iv; f.read_off = read_off; f.sel_off = sel_off; f.sel = sel; f.n_sel = n_sel;
    f.n_reads = n_reads; f.base_cap = base_capacity; f.cigar_cap = cigar_capacity;
    f.read_pos = (int64_t*)out->read_pos; f.base_off = (int64_t*)out->base_off; f.cigar_off = (int64_t*)out->cigar_off;
    f.read_flags = (uint8_t*)out->read_flags; f.read_mapq = (uint8_t*)out->read_mapq;
    f.bases = (uint8_t*)out->bases; f.quals = (uint8_t*)out->quals; f.cigar = (uint32_t*)out->cigar;
    f.read_hp = read_hp; f.totals = d_totals;
    k_bam_gather<<<(unsigned)((n_reads + 255) / 256), 256, 0, st>>>(*in, w, f);
    k_bam_offsets<<<1, 1024, 0, st>>>(w, f);
    const int64_t waves = n_reads < 16384 ? n_reads : 16384;
    k_bam_fill<<<(unsigned)((waves + 3) / 4), 256, 0, st>>>(*in, w, f);
    PV_HIP(hipGetLastError());
    return PV_OK;
}
