// polish_vote.hip — the polisher without a model: the builder's ten raw read counts and depth of every chunk row + draft bytes
// -> the labels (and the accumulated "softmax") the network would have left, by a majority of the reads of the row itself.
//
// The rule is in include/pepper_hip.h (pv_polish_vote). It stands where pv_rnn_forward_p2_dev stands in the chain and writes
// the same two planes, labels [n_chunks][L] and acc [n_chunks][L][5], so the row qualities, the mask, the filters, the
// stitch and the edits behind it need no change. Every row is treated, owned or not: rows two chunks share carry the same
// counts, depth and draft byte and so get the same label.
//
// Three launches as in the mask, no global atomics: per-chunk sums and the verdict on the chunk (one block per chunk), one
// block folding them into d_counts, then the write pass, which runs only under status PV_OK: a call that reports
// PV_ERR_INVALID has written nothing but d_counts. A counts row is loaded as five dwords (counts_row). acc is 20 bytes a
// row: the write pass leaves the five floats of its 256 rows in LDS and the lanes then store consecutive dwords, so a wave's
// store covers 256 contiguous bytes where a lane's own 20-byte stride would touch five times as many lines.
#include "polish_stitch_common.hpp"

using namespace pv_chunks;

namespace {

// what the vote kernels read and write beside the stitch's arguments (a.lab is not read: there are no labels yet)
struct VoteArgs {
    const uint16_t* depth;
    const uint16_t* rowc;      // chunks->counts, [row][10]
    const int64_t* ref_off;
    const uint8_t* ref;
    uint8_t* lab_out;
    float* acc;                // may be null: not written
    int overlap;
    int32_t* chunk_nr;         // [n_chunks] base rows without reads (a.chunk_cnt: rows changed, a.chunk_bad: BAD_ codes)
};

enum { ROW_PAD = 0, ROW_VOTED = 1, ROW_BAD_POS = 2 };

// the verdict on one row: its label, the reads behind each label and their sum, and what d_counts counts
struct Vote {
    int kind;                      // ROW_ code
    int label;
    uint32_t n0, n1, n2, n3, n4;   // reads that spell nothing (a deletion; no inserted base), A, C, G, T
    uint32_t total;
    bool changed, no_reads;        // the winner is not what the draft holds; a base row with total == 0
};

// rs, draft, span: the start of the chunk's region and the bytes of its draft. The draft byte is loaded for index-0 rows
// only, inside [0, span); the counts row and the depth for rows that are not padding.
__device__ inline Vote vote_row(const StitchArgs& a, const VoteArgs& m, int64_t t, int64_t rs, const uint8_t* draft, int64_t span) {
    Vote v;
    v.kind = ROW_PAD; v.label = 0; v.n0 = v.n1 = v.n2 = v.n3 = v.n4 = 0; v.total = 0; v.changed = false; v.no_reads = false;
    const int64_t p = a.pos[t];
    const int32_t x = a.idx[t];
    if (p < 0 || x < 0) return v;
    uint32_t dl = 0;   // 1..4: the label that spells the draft byte; 0: none does (base rows), nothing (insert rows)
    if (x == 0) {
        const int64_t rel = p - rs;
        if (rel < 0 || rel >= span) { v.kind = ROW_BAD_POS; return v; }
        const uint32_t d = draft[rel];
        const uint32_t u = d >= 'a' && d <= 'z' ? d - 32 : d;
        dl = (acgt_index(u) + 1) % 5;
    }
    v.kind = ROW_VOTED;
    const CountsRow w = counts_row(m.rowc, t);
    v.n1 = (w.w0 & 0xFFFFu) + (w.w2 & 0xFFFFu);
    v.n2 = (w.w0 >> 16) + (w.w2 >> 16);
    v.n3 = (w.w1 & 0xFFFFu) + (w.w3 & 0xFFFFu);
    v.n4 = (w.w1 >> 16) + (w.w3 >> 16);
    const uint32_t other = (w.w4 & 0xFFFFu) + (w.w4 >> 16), sum10 = v.n1 + v.n2 + v.n3 + v.n4 + other;
    const uint32_t top = max(max(v.n1, v.n2), max(v.n3, v.n4));
    const uint32_t first = v.n1 == top ? 1u : v.n2 == top ? 2u : v.n3 == top ? 3u : 4u;   // the smallest of the best bases
    if (x == 0) {
        v.n0 = other;
        v.total = sum10;
        const uint32_t n_dl = dl == 1 ? v.n1 : dl == 2 ? v.n2 : dl == 3 ? v.n3 : dl == 4 ? v.n4 : 0u;
        if (v.total == 0) v.label = (int)dl;                    // no reads: the draft, or nothing where no label spells it
        else if (v.n0 > top) v.label = 0;                       // a deletion wins only strictly ahead of every base
        else v.label = dl && n_dl == top ? (int)dl : (int)first;
        v.changed = dl == 0 || (uint32_t)v.label != dl;
        v.no_reads = v.total == 0;
    } else {
        const uint32_t d = m.depth[t];
        v.n0 = (d > sum10 ? d - sum10 : 0u) + other;            // reads over the anchor that hold nothing here, or no ACGT
        v.total = v.n0 + v.n1 + v.n2 + v.n3 + v.n4;
        v.label = v.n0 >= top ? 0 : (int)first;                 // on a tie nothing, which is the draft, wins
        v.changed = v.label != 0;
    }
    return v;
}

// one block per chunk: the rows whose winner is not the draft's, the base rows without reads, and whether the chunk breaks
// the layout (a base position outside the region's draft counts as that)
__global__ __launch_bounds__(ST_THREADS) void k_vote_count(StitchArgs a, VoteArgs m) {
    __shared__ int32_t lds[ST_THREADS / 64];
    const int64_t k = blockIdx.x;
    const bool ordered = chunk_in_order(a, k);
    int n = 0, nr = 0, bad_pos = 0;
    if (ordered) {
        const int32_t g = a.region[k];
        const int64_t rs = a.rstart[g], o0 = m.ref_off[g], span = m.ref_off[g + 1] - o0;
        const int64_t base = k * a.L;
        for (int j = threadIdx.x; j < a.L; j += ST_THREADS) {
            const Vote v = vote_row(a, m, base + j, rs, m.ref + o0, span);
            n += v.changed;
            nr += v.no_reads;
            bad_pos |= v.kind == ROW_BAD_POS;
        }
    }
    int32_t total, n_nr, npos;
    block_excl_scan<ST_THREADS, int32_t>(n, lds, &total);
    block_excl_scan<ST_THREADS, int32_t>(nr, lds, &n_nr);
    block_excl_scan<ST_THREADS, int32_t>(bad_pos, lds, &npos);
    if (threadIdx.x == 0) {
        a.chunk_cnt[k] = total;
        m.chunk_nr[k] = n_nr;
        a.chunk_bad[k] = (!ordered || npos) ? BAD_ORDER : BAD_NONE;
    }
}

// one block per chunk, under status PV_OK only: every row's label, and its five fractions where acc is given
__global__ __launch_bounds__(ST_THREADS) void k_vote_write(StitchArgs a, VoteArgs m) {
#pragma clang fp contract(off)
    __shared__ float s_acc[ST_THREADS * 5];
    if (a.counts[1] != PV_OK) return;
    const int64_t k = blockIdx.x;
    const int32_t g = a.region[k];
    const int64_t rs = a.rstart[g], o0 = m.ref_off[g], span = m.ref_off[g + 1] - o0;
    const int64_t base = k * a.L;
    for (int j0 = 0; j0 < a.L; j0 += ST_THREADS) {   // (the trip count and m.acc are the block's: the barriers are met by all)
        const int j = j0 + (int)threadIdx.x;
        if (j < a.L) {
            const Vote v = vote_row(a, m, base + j, rs, m.ref + o0, span);   // (status OK: no ROW_BAD_POS can come back)
            m.lab_out[base + j] = (uint8_t)v.label;
            if (m.acc) {
                // one correctly rounded divide, then a multiply by 1 or 2: pv_polish_row_qual's acc / cnt is n / total again
                const float wj = (j < m.overlap || j >= a.L - m.overlap) ? 1.0f : 2.0f;
                const float tot = (float)max(v.total, 1u);
                float* s = s_acc + threadIdx.x * 5;   // (the lanes' stride of 5 dwords spreads over the banks)
                s[0] = wj * ((float)v.n0 / tot);
                s[1] = wj * ((float)v.n1 / tot);
                s[2] = wj * ((float)v.n2 / tot);
                s[3] = wj * ((float)v.n3 / tot);
                s[4] = wj * ((float)v.n4 / tot);
            }
        }
        if (m.acc) {
            __syncthreads();
            const int nf = min(ST_THREADS, a.L - j0) * 5;
            float* dst = m.acc + (base + j0) * 5;
            for (int i = threadIdx.x; i < nf; i += ST_THREADS) dst[i] = s_acc[i];
            __syncthreads();   // s_acc is filled again in the next round
        }
    }
}

// what both forms refuse before they touch the device
int vote_check(const pv_polish_out* chunks, int64_t n_chunks, const uint8_t* ref, int seq_length, int seq_overlap) {
    PV_CHECK(n_chunks >= 0 && seq_length >= 1, PV_ERR_INVALID, "negative sizes");
    PV_CHECK(seq_overlap >= 0 && 2 * (int64_t)seq_overlap <= seq_length, PV_ERR_INVALID,
             "vote: need 0 <= 2 * seq_overlap <= seq_length (got %d, %d)", seq_length, seq_overlap);
    PV_CHECK(n_chunks == 0 || (chunks->depth && chunks->counts), PV_ERR_INVALID,
             "vote: the chunks carry no depth plane or no counts plane (pv_polish_out.depth, .counts)");
    PV_CHECK(n_chunks == 0 || ref, PV_ERR_INVALID, "vote: the batch carries no draft bytes (ref is null)");
    return PV_OK;
}

}  // namespace

extern "C" int pv_polish_vote_dev(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const int64_t* region_start,
                                  const int64_t* ref_off, const uint8_t* ref, int32_t n_regions, int seq_length, int seq_overlap,
                                  uint8_t* labels, float* acc, int64_t* d_counts, void* stream) {
    PV_CHECK(ctx && chunks && d_counts, PV_ERR_INVALID, "null argument");
    PV_CHECK(n_regions >= 0, PV_ERR_INVALID, "negative sizes");
    int rc;
    if ((rc = vote_check(chunks, n_chunks, ref, seq_length, seq_overlap))) return rc;
    PV_CHECK(((uintptr_t)chunks->counts & 3) == 0, PV_ERR_INVALID, "counts is not aligned to 4 bytes");
    PV_CHECK(((uintptr_t)acc & 3) == 0, PV_ERR_INVALID, "acc is not aligned to a float");
    PV_CHECK(n_chunks <= chunks->chunk_capacity, PV_ERR_INVALID, "n_chunks %lld exceeds the chunk capacity %lld",
             (long long)n_chunks, (long long)chunks->chunk_capacity);
    PV_CHECK(n_chunks < (1ll << 31), PV_ERR_LIMIT, "too many chunks for one launch");
    PV_CHECK(n_chunks == 0 || (chunks->position && chunks->index && chunks->region && chunks->chunk_id && labels && region_start &&
                               ref_off && n_regions > 0),
             PV_ERR_INVALID, "chunk arrays, labels, region starts or draft offsets missing");
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = pv_pick_stream(ctx, stream);
    StitchArgs a = chunk_args(chunks, nullptr, region_start, n_chunks, n_regions, seq_length, seq_overlap, d_counts);
    VoteArgs m = {chunks->depth, chunks->counts, ref_off, ref, labels, acc, seq_overlap, nullptr};
    const size_t nk = (size_t)(n_chunks > 0 ? n_chunks : 1);
    if ((rc = pv_get(ctx, "vote.cnt", nk, &a.chunk_cnt))) return rc;
    if ((rc = pv_get(ctx, "vote.bad", nk, &a.chunk_bad))) return rc;
    if ((rc = pv_get(ctx, "vote.nr", nk, &m.chunk_nr))) return rc;
    pv_prof_scope ps_all(ctx, "polish_vote", st);
    if (n_chunks > 0) { pv_prof_scope ps(ctx, "k_vote_count", st); k_vote_count<<<(unsigned)n_chunks, ST_THREADS, 0, st>>>(a, m); }
    k_chunk_finish<<<1, ST_FINISH_THREADS, 0, st>>>(a, m.chunk_nr);
    if (n_chunks > 0) { pv_prof_scope ps(ctx, "k_vote_write", st); k_vote_write<<<(unsigned)n_chunks, ST_THREADS, 0, st>>>(a, m); }
    PV_HIP(hipGetLastError());
    return PV_OK;
}

extern "C" int pv_polish_vote(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const int64_t* region_start,
                              const int64_t* ref_off, const uint8_t* ref, int32_t n_regions, int seq_length, int seq_overlap,
                              uint8_t* labels, float* acc, int64_t* counts) {
    PV_CHECK(ctx && chunks && counts, PV_ERR_INVALID, "null argument");
    PV_CHECK(n_regions >= 0, PV_ERR_INVALID, "negative sizes");
    int rc;   // everything the call itself refuses is refused here, before a byte is copied to the device
    if ((rc = vote_check(chunks, n_chunks, ref, seq_length, seq_overlap))) return rc;
    PV_CHECK(n_chunks == 0 || (ref_off && n_regions > 0), PV_ERR_INVALID, "draft offsets missing");
    PV_CHECK(n_chunks == 0 || labels, PV_ERR_INVALID, "labels missing");
    PV_CHECK(!ref_off || ref_off[n_regions] >= 0, PV_ERR_INVALID, "negative draft length");
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t nc = (size_t)n_chunks, L = (size_t)seq_length;
    pv_polish_out d;
    uint8_t *d_lab = nullptr, *d_ref = nullptr;
    float* d_acc = nullptr;
    int64_t *d_rs = nullptr, *d_ro = nullptr, *d_counts = nullptr;
    if ((rc = stage_chunks(ctx, "vt", chunks, nc, L, true, true, &d, st))) return rc;
    if ((rc = stage_draft(ctx, "vt", region_start, ref_off, ref, n_regions, &d_rs, &d_ro, &d_ref, st))) return rc;
    if ((rc = pv_get(ctx, "vt.labels", nc * L > 0 ? nc * L : 1, &d_lab))) return rc;
    if (acc && (rc = pv_get(ctx, "vt.acc", nc * L > 0 ? nc * L * 5 : 1, &d_acc))) return rc;
    if ((rc = pv_get(ctx, "vt.counts", (size_t)4, &d_counts))) return rc;
    rc = pv_polish_vote_dev(ctx, &d, n_chunks, d_rs, d_ro, d_ref, n_regions, seq_length, seq_overlap, d_lab, acc ? d_acc : nullptr,
                            d_counts, st);
    if (rc) return rc;
    PV_HIP(hipMemcpyAsync(counts, d_counts, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    PV_HIP(hipStreamSynchronize(st));
    const int64_t status = counts[1];
    PV_CHECK(status != PV_ERR_INVALID, PV_ERR_INVALID,
             "vote: chunk %lld breaks the layout (regions ascending, chunk ids 0,1,2,... inside a region, base positions inside "
             "the region's draft bytes)", (long long)counts[2]);
    PV_CHECK(status == PV_OK, (int)status, "vote: device status %lld", (long long)status);
    if (nc * L > 0) {
        PV_HIP(hipMemcpyAsync(labels, d_lab, nc * L, hipMemcpyDeviceToHost, st));
        if (acc) PV_HIP(hipMemcpyAsync(acc, d_acc, nc * L * 5 * sizeof(float), hipMemcpyDeviceToHost, st));
        PV_HIP(hipStreamSynchronize(st));
    }
    return PV_OK;
}
