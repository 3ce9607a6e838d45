// summary_polish.hip — the polisher's (P2) summary images: k_polish_* behind the shared front end of summary_front.hip.
#include "summary_launch.hpp"

namespace pvsum {
namespace {

// ==== P2 (polisher) summary images ====================================================================
// SummaryGenerator::iterate_over_read / generate_image (pepper/modules/src/pileup_summary/summary_generator.cpp:47-121,
// 274-304). Same tile-owner scheme as k_pileup_tiles (pairs -> ops -> bases, counters of a 512-column tile in LDS), with
// the polisher's much simpler per-base rule: one ds_add into one of ten (symbol, strand) planes, no qualities.
constexpr int PC_COV = 10, PC_LONG = 11, PC_N = 12;  // global planes: 0-9 features, coverage, longest insert
enum { Q_F = 0, Q_STAR = 10 /* [rev, fwd] deleted columns */, Q_DCOV = 12, Q_LONG = 13, Q_N = 14 };

// get_feature_index (summary_generator.cpp:16-33): toupper, then reverse A0 C1 G2 T3 else 8, forward A4 C5 G6 T7 else 9
__device__ __forceinline__ int polish_sym(int c) { c = up(c); return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4; }
__device__ __forceinline__ int polish_feature(int sym, bool rev) { return sym < 4 ? (rev ? sym : 4 + sym) : (rev ? 8 : 9); }

__global__ __launch_bounds__(PT_THREADS) void k_polish_tiles(SumArgs a) {
    __shared__ int32_t s_cnt[Q_N][TILE_COLS];
    __shared__ uint8_t s_lut[256];           // polish_sym of every byte
    __shared__ uint16_t s_blk[PT_THREADS * (TILE_COLS + 4) / 64 + 2];
    __shared__ int32_t s_pref[PT_THREADS];   // inclusive prefix of in-tile aligned bases, every op padded to whole groups of 4
    __shared__ int32_t s_iend[PT_THREADS];
    __shared__ int32_t s_col0[PT_THREADS];
    __shared__ int64_t s_base[PT_THREADS];
    __shared__ int32_t s_i0[PT_THREADS];
    __shared__ uint8_t s_opfl[PT_THREADS];   // bit0 rev
    __shared__ uint8_t s_opair[PT_THREADS];
    __shared__ int32_t p_off[PT_PB + 1];
    __shared__ int32_t p_oplo[PT_PB], p_colbase[PT_PB], p_R[PT_PB], p_rev[PT_PB];
    __shared__ int64_t p_base0[PT_PB], p_seqend[PT_PB];
    __shared__ int32_t s_wsum[2 * (PT_THREADS / 64)];
    int scan_turn = 0;
    const int tid = threadIdx.x;
    const int64_t tile = blockIdx.x;
    const int64_t tlo = tile * TILE_COLS, thi = tlo + TILE_COLS - 1;
    for (int i = tid; i < Q_N * TILE_COLS; i += PT_THREADS) (&s_cnt[0][0])[i] = 0;
    if (tid < 256) s_lut[tid] = (uint8_t)polish_sym(tid);
    const int32_t p0 = a.tile_off[tile];
    const int32_t np = a.tile_cnt[tile];
    __syncthreads();
    for (int32_t pb = 0; pb < np; pb += PT_PB) {
        const int npb = (np - pb) < PT_PB ? (np - pb) : PT_PB;
        int nops = 0;
        if (tid < npb) {
            const PairRec pr = a.pairs[p0 + pb + tid];
            nops = pr.op_hi - pr.op_lo;
            p_oplo[tid] = pr.op_lo; p_colbase[tid] = pr.col_base; p_R[tid] = pr.R;
            p_rev[tid] = pr.rev; p_base0[tid] = pr.base0; p_seqend[tid] = pr.seq_end;
        }
        const int incl_ops = block_incl_scan512(nops, s_wsum, tid, scan_turn);
        if (tid < npb) p_off[tid + 1] = incl_ops;
        if (tid == 0) p_off[0] = 0;
        __syncthreads();
        const int total_ops = p_off[npb];
        for (int ob = 0; ob < total_ops; ob += PT_THREADS) {
            const int k = ob + tid;
            int32_t ref_rel = 0, rd = 0, len = 0, op = 15, col_base = 0, R = 0;
            bool active = false, rev = false;
            int pslot = 0;
            int32_t c = 0;
            int64_t clo = 0, chi = -1;
            if (k < total_ops) {
                int lo = 0, hi = npb;
                while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (p_off[mid] <= k) lo = mid; else hi = mid; }
                pslot = lo;
                c = p_oplo[pslot] + (k - p_off[pslot]);
                const int32_t rr = a.op_ref[c];
                const uint32_t w = a.in.cigar[c];
                const int32_t rdv = a.op_rd[c];
                col_base = p_colbase[pslot];
                rev = p_rev[pslot] != 0;
                R = p_R[pslot];
                active = rr != OP_INACTIVE;
                if (active) { ref_rel = rr; rd = rdv; op = w & 0xF; len = (int32_t)(w >> 4); }
                clo = tlo - col_base; chi = thi - col_base;
                if (clo < 0) clo = 0;
                if (chi > R - 1) chi = R - 1;
            }
            if (active && op == PV_CIGAR_IN) {  // :82-98; the tile that owns the anchor column takes the op
                const int64_t anchor = (int64_t)ref_rel - 1;
                if (anchor >= clo && anchor <= chi) {
                    const int lc = (int)(col_base + anchor - tlo);
                    if (p_base0[pslot] + rd + (int64_t)len > p_seqend[pslot]) {
                        set_status(a.diag, PV_ERR_INVALID);  // alt[i] past the end of the read
                    } else {
                        atomicMax(&s_cnt[Q_LONG][SW(lc)], len);
                        a.op_flag[c] = 1;  // counted per insert row by k_polish_insert once the row layout is known
                    }
                }
            } else if (active && (op == PV_CIGAR_DEL || op == PV_CIGAR_REF_SKIP || op == PV_CIGAR_PAD)) {  // :100-114
                int64_t i0 = clo - ref_rel; if (i0 < 0) i0 = 0;
                int64_t i1 = chi + 1 - ref_rel; if (i1 > len) i1 = len;
                for (int64_t i = i0; i < i1; i++)
                    atomicAdd(&s_cnt[Q_STAR + (rev ? 0 : 1)][SW((int)((int64_t)col_base + ref_rel + i - tlo))], 1);
                // "coverage[ref_position] += 1.0" sits INSIDE the loop over the deleted columns but is keyed by the
                // START of the deletion (:110): that column gains one per in-region deleted column, the others nothing.
                if ((int64_t)ref_rel >= clo && (int64_t)ref_rel <= chi) {
                    int64_t n = (int64_t)R - ref_rel; if (n > len) n = len;
                    if (n > 0) atomicAdd(&s_cnt[Q_DCOV][SW((int)(col_base + ref_rel - tlo))], (int)n);
                }
            }
            const bool is_m = active && (op == PV_CIGAR_MATCH || op == PV_CIGAR_EQUAL || op == PV_CIGAR_DIFF);
            int32_t i0 = 0, eff = 0;
            if (is_m) {
                int64_t lo = clo - ref_rel; if (lo < 0) lo = 0;
                int64_t hi = chi + 1 - ref_rel; if (hi > len) hi = len;
                if (hi > lo) { i0 = (int32_t)lo; eff = (int32_t)(hi - lo); }
            }
            const int32_t effp = (eff + 3) & ~3;  // groups of 4 slots never straddle two ops (see k_pileup_tiles)
            const int32_t incl = block_incl_scan512(effp, s_wsum, tid, scan_turn);
            s_pref[tid] = incl;
            s_col0[tid] = col_base + ref_rel;
            s_base[tid] = (k < total_ops ? p_base0[pslot] : 0) + rd;
            s_i0[tid] = i0 - (incl - effp);
            s_iend[tid] = i0 + eff;
            s_opfl[tid] = (uint8_t)(rev ? 1 : 0);
            s_opair[tid] = (uint8_t)pslot;
            for (int32_t bb = (incl - effp + 63) >> 6; (bb << 6) < incl; bb++) s_blk[bb] = (uint16_t)tid;
            __syncthreads();
            const int32_t total = s_pref[PT_THREADS - 1];
            for (int32_t jb = 0; jb < total; jb += PT_THREADS * PT_GPL * 4) {
                int lcv[PT_GPL], nvv[PT_GPL], rv[PT_GPL];
                uint32_t bw[PT_GPL];
#pragma unroll
                for (int u = 0; u < PT_GPL; u++) {
                    const int32_t j = jb + (u * PT_THREADS + tid) * 4;
                    const bool ok = j < total;
                    int owc = ok ? s_blk[j >> 6] : 0;
                    while (ok && s_pref[owc] <= j) owc++;
                    const int32_t i = j + s_i0[owc];
                    int nv = s_iend[owc] - i;
                    nv = ok ? (nv > 4 ? 4 : nv) : 0;
                    const int64_t bi = s_base[owc] + i;
                    const int64_t left = p_seqend[s_opair[owc]] - bi;
                    if (nv > 0 && nv > left) { set_status(a.diag, PV_ERR_INVALID); nv = left > 0 ? (int)left : 0; }
                    lcv[u] = (int)((int64_t)s_col0[owc] + i - tlo);
                    nvv[u] = nv;
                    rv[u] = s_opfl[owc] & 1;
                    uint32_t b4 = 0;
                    if (nv > 0) {
                        if (bi + 4 <= a.n_bases) b4 = *reinterpret_cast<const uint32_t*>(a.in.bases + bi);
                        else for (int e = 0; e < nv; e++) b4 |= (uint32_t)a.in.bases[bi + e] << (8 * e);
                    }
                    bw[u] = b4;
                }
#pragma unroll
                for (int u = 0; u < PT_GPL; u++) {
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        if (e >= nvv[u]) continue;
                        atomicAdd(&s_cnt[Q_F + polish_feature(s_lut[(bw[u] >> (8 * e)) & 0xFF], rv[u] != 0)][SW(lcv[u] + e)], 1);  // :70-74
                    }
                }
            }
            __syncthreads();
        }
        __syncthreads();
    }
    __syncthreads();
    const int64_t NC = a.n_cols;
    int64_t ncol = NC - tlo;
    if (ncol > TILE_COLS) ncol = TILE_COLS;
    for (int lc = tid; lc < ncol; lc += PT_THREADS) {
        const int64_t g = tlo + lc;
        int cov = s_cnt[Q_DCOV][SW(lc)];
#pragma unroll
        for (int f = 0; f < 10; f++) {
            const int v = s_cnt[Q_F + f][SW(lc)];
            cov += v;  // every aligned base bumps coverage once (:72-73)
            a.pcnt[(int64_t)f * NC + g] = v + (f == 8 ? s_cnt[Q_STAR][SW(lc)] : f == 9 ? s_cnt[Q_STAR + 1][SW(lc)] : 0);
        }
        a.pcnt[(int64_t)PC_COV * NC + g] = cov;
        a.pcnt[(int64_t)PC_LONG * NC + g] = s_cnt[Q_LONG][SW(lc)];
    }
}

// insert rows per 1024-column block (columns of the reference buffer beyond R never get an insert: the tile kernel clips)
__global__ __launch_bounds__(1024) void k_polish_blk(SumArgs a) {
    __shared__ int32_t s_w[16];
    const int64_t col = (int64_t)blockIdx.x * 1024 + threadIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int32_t v = col < a.n_cols ? a.pcnt[(int64_t)PC_LONG * a.n_cols + col] : 0;
    const int32_t inc = wave_incl_scan32(v, lane);
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    if (threadIdx.x == 0) { int32_t t = 0; for (int k = 0; k < 16; k++) t += s_w[k]; a.ins_blk[blockIdx.x] = t; }
}

__global__ __launch_bounds__(1024) void k_polish_insoff(SumArgs a) {
    __shared__ int32_t s_w[16];
    const int64_t col = (int64_t)blockIdx.x * 1024 + threadIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int32_t v = col < a.n_cols ? a.pcnt[(int64_t)PC_LONG * a.n_cols + col] : 0;
    const int32_t inc = wave_incl_scan32(v, lane);
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    int32_t woff = 0;
    for (int k = 0; k < wv; k++) woff += s_w[k];
    const int32_t excl = a.ins_blkoff[blockIdx.x] + woff + inc - v;
    if (col < a.n_cols) a.ins_off[col] = excl;
    if (col == a.n_cols - 1) a.ins_off[a.n_cols] = excl + v;
}

// row / chunk layout of the regions (sequential over the few regions of a batch), limits, counters
__global__ void k_polish_regions(SumArgs a) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int64_t rows = 0, chunks = 0;
    for (int g = 0; g < a.in.n_regions; g++) {
        a.reg_rows[g] = rows;
        a.reg_chunks[g] = chunks;
        const int64_t R = a.in.ref_end[g] - a.in.ref_start[g] + 1;
        const int64_t c0 = a.in.ref_off[g];
        const int64_t n = R + (a.ins_off[c0 + R] - a.ins_off[c0]);
        rows += n;
        // AlignmentSummarizer.chunk_images (AlignmentSummarizer.py:19-56): starts 0, L-O, 2(L-O), ... until a chunk ends at n
        chunks += n <= a.seq_len ? 1 : 1 + (n - a.seq_len + a.seq_step - 1) / a.seq_step;
    }
    a.reg_rows[a.in.n_regions] = rows;
    a.reg_chunks[a.in.n_regions] = chunks;
    a.diag[D_NROWS] = rows;
    a.diag[D_NCHUNKS] = chunks;
    if (a.diag[D_NINS] > a.max_ins_rows) set_status(a.diag, PV_ERR_LIMIT);
    a.d_counts[0] = chunks;
    a.d_counts[1] = rows;
    a.d_counts[2] = a.diag[D_STATUS];
    a.d_counts[3] = a.diag[D_NINS];
}

// thread per CIGAR op: the bases of every in-region insert, counted on its insert rows (:88-93)
__global__ __launch_bounds__(256) void k_polish_insert(SumArgs a) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= a.n_cigar || a.diag[D_STATUS] != 0 || a.op_flag[c] != 1) return;
    const uint32_t w = a.in.cigar[c];
    const int32_t len = (int32_t)(w >> 4);
    const int32_t r = a.op_read[c];
    const int g = a.read_region[r];
    const int64_t col = a.in.ref_off[g] + a.op_ref[c] - 1;
    const int64_t row = a.ins_off[col];
    const int64_t b0 = a.in.base_off[r] + a.op_rd[c];
    const bool rev = (a.in.read_flags[r] & 1) != 0;
    for (int32_t i = 0; i < len; i++)
        atomicAdd(&a.ins_cnt[(row + i) * 10 + polish_feature(polish_sym(a.in.bases[b0 + i]), rev)], 1);
}

__device__ __forceinline__ uint8_t polish_pixel(int32_t cnt, int32_t cov) {  // generate_image, :281 / :293-294
    const double v = ((double)cnt / ((double)cov > 1.0 ? (double)cov : 1.0)) * 254.0;
    return (uint8_t)(uint32_t)(int32_t)v;
}

// ten counts -> the 20 bytes of a counts row (pv_polish_out.counts), clamped to uint16, as five dwords: the row is 4-byte aligned
__device__ __forceinline__ uint32_t cnt16(int32_t v) { return (uint32_t)(v > 65535 ? 65535 : v); }
__device__ __forceinline__ void store_counts_row(uint16_t* row, const int32_t* c) {
    uint32_t* d = reinterpret_cast<uint32_t*>(row);
#pragma unroll
    for (int w = 0; w < 5; w++) d[w] = cnt16(c[2 * w]) | cnt16(c[2 * w + 1]) << 16;
}

// thread per column: its base row and its insert rows. COUNTS: also the raw counts of every row (a.flat_counts); the
// instantiation without them is the kernel as it was
template <bool COUNTS>
__global__ __launch_bounds__(256) void k_polish_image(SumArgs a) {
    const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (col >= a.n_cols || a.diag[D_STATUS] != 0) return;
    const int g = upper_bound_i64(a.in.ref_off, a.in.n_regions + 1, col) - 1;
    if (g < 0 || g >= a.in.n_regions) return;
    const int64_t c0 = a.in.ref_off[g];
    const int64_t i = col - c0;
    if (i >= a.in.ref_end[g] - a.in.ref_start[g] + 1) return;
    const int64_t NC = a.n_cols;
    const int64_t ins0 = a.ins_off[col];
    int64_t row = a.reg_rows[g] + i + (ins0 - a.ins_off[c0]);
    const int32_t cov = a.pcnt[(int64_t)PC_COV * NC + col];
    const int32_t nl = a.pcnt[(int64_t)PC_LONG * NC + col];
    const int64_t pos = a.in.ref_start[g] + i;
    // the depth plane (pv_polish_out.depth): the column's ten counts, summed; its insert rows take the same value
    uint16_t depth = 0;
    if (a.flat_depth) {
        int32_t d = 0;
#pragma unroll
        for (int f = 0; f < 10; f++) d += a.pcnt[(int64_t)f * NC + col];
        depth = (uint16_t)(d > 65535 ? 65535 : d);
    }
    if (row < a.flat_cap) {
#pragma unroll
        for (int f = 0; f < 10; f++) a.flat_img[row * 10 + f] = polish_pixel(a.pcnt[(int64_t)f * NC + col], cov);
        a.flat_pos[row] = pos;
        a.flat_idx[row] = 0;
        if (a.flat_depth) a.flat_depth[row] = depth;
        if (COUNTS) {
            int32_t c[10];
#pragma unroll
            for (int f = 0; f < 10; f++) c[f] = a.pcnt[(int64_t)f * NC + col];
            store_counts_row(a.flat_counts + row * 10, c);
        }
    }
    for (int32_t ii = 0; ii < nl; ii++) {
        row++;
        if (row >= a.flat_cap) break;
#pragma unroll
        for (int f = 0; f < 10; f++) a.flat_img[row * 10 + f] = polish_pixel(a.ins_cnt[(ins0 + ii) * 10 + f], cov);
        a.flat_pos[row] = pos;
        a.flat_idx[row] = ii + 1;
        if (a.flat_depth) a.flat_depth[row] = depth;
        if (COUNTS) store_counts_row(a.flat_counts + row * 10, a.ins_cnt + (ins0 + ii) * 10);
    }
}

// thread per (chunk, row): gather from the flat rows, or pad. COUNTS: the counts row too, five dwords
template <bool COUNTS>
__global__ __launch_bounds__(256) void k_polish_chunks(SumArgs a) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (a.diag[D_STATUS] != 0) return;
    int64_t nck = a.diag[D_NCHUNKS];
    if (nck > a.pout.chunk_capacity) nck = a.pout.chunk_capacity;
    const int64_t k = t / a.seq_len;
    if (k >= nck) return;
    const int j = (int)(t - k * a.seq_len);
    const int g = upper_bound_i64(a.reg_chunks, a.in.n_regions + 1, k) - 1;
    const int64_t kk = k - a.reg_chunks[g];
    const int64_t rows = a.reg_rows[g + 1] - a.reg_rows[g];
    const int64_t r = kk * a.seq_step + j;
    if (j == 0) { a.pout.region[k] = g; a.pout.chunk_id[k] = (int32_t)kk; }
    uint8_t* dst = a.pout.images + t * 10;
    if (r < rows && a.reg_rows[g] + r < a.flat_cap) {
        const int64_t src = a.reg_rows[g] + r;
#pragma unroll
        for (int f = 0; f < 10; f++) dst[f] = a.flat_img[src * 10 + f];
        a.pout.position[t] = a.flat_pos[src];
        a.pout.index[t] = a.flat_idx[src];
        if (a.pout.depth) a.pout.depth[t] = a.flat_depth[src];
        if (COUNTS) {
            const uint32_t* cs = reinterpret_cast<const uint32_t*>(a.flat_counts + src * 10);
            uint32_t* cd = reinterpret_cast<uint32_t*>(a.pout.counts + t * 10);
#pragma unroll
            for (int w = 0; w < 5; w++) cd[w] = cs[w];
        }
    } else {
#pragma unroll
        for (int f = 0; f < 10; f++) dst[f] = 0;
        a.pout.position[t] = -1;
        a.pout.index[t] = -1;
        if (a.pout.depth) a.pout.depth[t] = 0;
        if (COUNTS) {
            uint32_t* cd = reinterpret_cast<uint32_t*>(a.pout.counts + t * 10);
#pragma unroll
            for (int w = 0; w < 5; w++) cd[w] = 0;
        }
    }
}

}  // namespace

// ==== P2 (polisher) summary images: launch sequence and C-ABI ===========================================
int polish_launch(pv_ctx* ctx, const pv_batch_in* in, int64_t n_reads, int64_t n_bases, int64_t n_cigar, int64_t n_cols,
                  int64_t max_pairs, int64_t max_ins_rows, int seq_length, int seq_overlap, const pv_polish_out* out,
                  int64_t* d_counts, hipStream_t st) {
    PV_CHECK(seq_length >= 1 && seq_overlap >= 0 && seq_overlap < seq_length, PV_ERR_INVALID,
             "need 0 <= seq_overlap < seq_length (got %d, %d)", seq_overlap, seq_length);
    SumArgs a;
    memset(&a, 0, sizeof(a));
    a.in = *in;
    a.polish = 1;
    a.seq_len = seq_length;
    a.seq_step = seq_length - seq_overlap;
    a.n_reads = n_reads; a.n_bases = n_bases; a.n_cigar = n_cigar; a.n_cols = n_cols;
    a.max_pairs = max_pairs;
    a.max_ins_rows = max_ins_rows;
    a.pout = *out;
    a.d_counts = d_counts;
    const int64_t n_blk = (n_cols + 1023) / 1024, G = in->n_regions;
    int rc;
    if ((rc = front_claim(ctx, a))) return rc;
    if ((rc = pv_get(ctx, "sum.op_read", (size_t)(n_cigar > 0 ? n_cigar : 1), &a.op_read))) return rc;
    if ((rc = pv_get(ctx, "pol.pcnt", (size_t)PC_N * n_cols, &a.pcnt))) return rc;
    if ((rc = pv_get(ctx, "pol.ins_blk", n_blk, &a.ins_blk))) return rc;
    if ((rc = pv_get(ctx, "pol.ins_blkoff", n_blk, &a.ins_blkoff))) return rc;
    if ((rc = pv_get(ctx, "pol.ins_off", n_cols + 1, &a.ins_off))) return rc;
    if ((rc = pv_get(ctx, "pol.ins_cnt", (size_t)(max_ins_rows > 0 ? max_ins_rows : 1) * 10, &a.ins_cnt))) return rc;
    if ((rc = pv_get(ctx, "pol.reg_rows", (size_t)G + 1, &a.reg_rows))) return rc;
    if ((rc = pv_get(ctx, "pol.reg_chunks", (size_t)G + 1, &a.reg_chunks))) return rc;
    if (out->flat_images) {
        PV_CHECK(out->flat_position && out->flat_index, PV_ERR_INVALID, "flat_position / flat_index missing");
        a.flat_img = out->flat_images; a.flat_pos = out->flat_position; a.flat_idx = out->flat_index;
        a.flat_cap = out->row_capacity;
    } else {
        a.flat_cap = n_cols + max_ins_rows;
        if ((rc = pv_get(ctx, "pol.flat_img", (size_t)a.flat_cap * 10, &a.flat_img))) return rc;
        if ((rc = pv_get(ctx, "pol.flat_pos", (size_t)a.flat_cap, &a.flat_pos))) return rc;
        if ((rc = pv_get(ctx, "pol.flat_idx", (size_t)a.flat_cap, &a.flat_idx))) return rc;
    }
    if (out->depth)   // the flat depth is workspace either way: pv_polish_out has no flat form of it
        if ((rc = pv_get(ctx, "pol.flat_depth", (size_t)(a.flat_cap > 0 ? a.flat_cap : 1), &a.flat_depth))) return rc;
    if (out->counts) {   // and so is the flat counts plane
        PV_CHECK(((uintptr_t)out->counts & 3) == 0, PV_ERR_INVALID, "counts is not aligned to 4 bytes");
        if ((rc = pv_get(ctx, "pol.flat_counts", (size_t)(a.flat_cap > 0 ? a.flat_cap : 1) * 10, &a.flat_counts))) return rc;
    }

    pv_prof_scope ps_all(ctx, "polish_pipeline", st);
    front_init(a, st);
    { int rcz = pv_zero_async(a.ins_cnt, (size_t)(max_ins_rows > 0 ? max_ins_rows : 1) * 10 * sizeof(int32_t), st); if (rcz) return rcz; }
    front_pairs(ctx, a, st);
    { pv_prof_scope ps(ctx, "k_polish_tiles", st); k_polish_tiles<<<(unsigned)a.n_tiles, PT_THREADS, 0, st>>>(a); }
    k_polish_blk<<<(unsigned)n_blk, 1024, 0, st>>>(a);
    front_scan_i32(a.ins_blk, a.ins_blkoff, n_blk, &a.diag[D_NINS], st);
    k_polish_insoff<<<(unsigned)n_blk, 1024, 0, st>>>(a);
    k_polish_regions<<<1, 1, 0, st>>>(a);
    if (n_cigar > 0) { pv_prof_scope ps(ctx, "k_polish_insert", st); k_polish_insert<<<grid_for(n_cigar, 256), 256, 0, st>>>(a); }
    {
        pv_prof_scope ps(ctx, "k_polish_image", st);
        if (a.flat_counts) k_polish_image<true><<<grid_for(n_cols, 256), 256, 0, st>>>(a);
        else k_polish_image<false><<<grid_for(n_cols, 256), 256, 0, st>>>(a);
    }
    if (out->chunk_capacity > 0 && out->images) {
        PV_CHECK(out->position && out->index && out->region && out->chunk_id, PV_ERR_INVALID, "chunk output arrays missing");
        pv_prof_scope ps(ctx, "k_polish_chunks", st);
        if (a.flat_counts) k_polish_chunks<true><<<grid_for(out->chunk_capacity * seq_length, 256), 256, 0, st>>>(a);
        else k_polish_chunks<false><<<grid_for(out->chunk_capacity * seq_length, 256), 256, 0, st>>>(a);
    }
    if (out->region_row_off)
        PV_HIP(hipMemcpyAsync(out->region_row_off, a.reg_rows, (size_t)(G + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    PV_HIP(hipGetLastError());
    return PV_OK;
}

void polish_limits(int64_t n_cols, int64_t n_bases, int64_t n_reads, int64_t* max_pairs, int64_t* max_ins_rows) {
    *max_pairs = 2 * (n_bases / TILE_COLS) + 3 * n_reads + 64;
    *max_ins_rows = 2 * n_cols + 4096;  // 60x ONT (2 % inserts of 1-3 bases) adds ~1.5 insert rows per column; the device reports overflow
}

}  // namespace pvsum

using namespace pvsum;

extern "C" int pv_polish_summarize_regions_dev(pv_ctx* ctx, const pv_batch_in* in, int64_t n_reads, int64_t n_bases,
                                               int64_t n_cigar, int64_t n_ref_bytes, int seq_length, int seq_overlap,
                                               pv_polish_out* out, int64_t* d_counts, void* stream) {
    PV_CHECK(ctx && in && out && d_counts, PV_ERR_INVALID, "null argument");
    PV_CHECK(in->n_regions >= 0 && n_ref_bytes >= 0, PV_ERR_INVALID, "negative sizes");
    PV_HIP(hipSetDevice(ctx->device));
    int64_t mp, mi;
    polish_limits(n_ref_bytes, n_bases, n_reads, &mp, &mi);
    if (out->flat_images && out->row_capacity > n_ref_bytes && out->row_capacity - n_ref_bytes > mi) mi = out->row_capacity - n_ref_bytes;
    return polish_launch(ctx, in, n_reads, n_bases, n_cigar, n_ref_bytes > 0 ? n_ref_bytes : 1, mp, mi, seq_length, seq_overlap,
                         out, d_counts, pv_pick_stream(ctx, stream));
}
