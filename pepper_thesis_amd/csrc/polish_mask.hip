// polish_mask.hip — the polisher's minimum depth: P2 labels + the builder's depth plane + draft bytes -> labels (and row
// qualities) that spell the draft wherever fewer than min_depth reads stand behind a row.
//
// The rule is in include/pepper_hip.h (pv_polish_mask_low_depth). It runs between the network and the stitch and rewrites
// labels only, so the stitch, quality and edit kernels behind it need no change and stay consistent with each other. Every row
// is treated, owned or not: rows two chunks share carry the same depth and draft byte and so get the same label.
//
// Three launches as in the edits, no global atomics: per-chunk counts and the verdict on the chunk (one block per chunk), one
// block folding them into d_counts, then the rewrite, which runs only under status PV_OK: a call that reports PV_ERR_INVALID
// has written nothing but d_counts, in place or not. A row's depth is loaded first; position, index and the draft byte are
// loaded by the lanes below min_depth only, so at a threshold few columns miss, both passes read little more than the depth
// plane, and in place the rewrite stores the masked rows alone.
#include "polish_stitch_common.hpp"

using namespace pv_chunks;

namespace {

// what the mask kernels read and write beside the stitch's arguments (a.lab: labels in)
struct MaskArgs {
    const uint16_t* depth;
    const uint8_t* qual;       // may be null, then qual_out is too
    const int64_t* ref_off;
    const uint8_t* ref;
    uint8_t* lab_out;
    uint8_t* qual_out;
    int min_depth;
    int32_t* chunk_unm;        // [n_chunks] unmaskable rows (a.chunk_cnt: masked rows, a.chunk_bad: BAD_ codes)
};

enum { ROW_COPY = -1, ROW_UNMASKABLE = -2, ROW_BAD_POS = -3 };

// >= 0: the row is masked and this is its label; else a ROW_ code. rs, draft, span: the start of the chunk's region and the
// bytes of its draft. The draft byte is loaded for masked index-0 rows only, inside [0, span).
__device__ inline int masked_label(const StitchArgs& a, const MaskArgs& m, int64_t t, int64_t rs, const uint8_t* draft, int64_t span) {
    if ((int)m.depth[t] >= m.min_depth) return ROW_COPY;
    const int64_t p = a.pos[t];
    if (p < 0) return ROW_COPY;
    const int32_t x = a.idx[t];
    if (x < 0) return ROW_COPY;
    if (x > 0) return 0;
    const int64_t rel = p - rs;
    if (rel < 0 || rel >= span) return ROW_BAD_POS;
    const uint32_t d = draft[rel];
    const uint32_t u = d >= 'a' && d <= 'z' ? d - 32 : d;
    return u == 'A' ? 1 : u == 'C' ? 2 : u == 'G' ? 3 : u == 'T' ? 4 : ROW_UNMASKABLE;
}

// one block per chunk: the rows it masks, the rows it cannot, and whether it breaks the layout (a masked position outside the
// region's draft counts as that)
__global__ __launch_bounds__(ST_THREADS) void k_mask_count(StitchArgs a, MaskArgs m) {
    __shared__ int32_t lds[ST_THREADS / 64];
    const int64_t k = blockIdx.x;
    const bool ordered = chunk_in_order(a, k);
    int n = 0, unm = 0, bad_pos = 0;
    if (ordered) {
        const int32_t g = a.region[k];
        const int64_t rs = a.rstart[g], o0 = m.ref_off[g], span = m.ref_off[g + 1] - o0;
        const int64_t base = k * a.L;
        for (int j = threadIdx.x; j < a.L; j += ST_THREADS) {
            const int r = masked_label(a, m, base + j, rs, m.ref + o0, span);
            n += r >= 0;
            unm += r == ROW_UNMASKABLE;
            bad_pos |= r == ROW_BAD_POS;
        }
    }
    int32_t total, nunm, npos;
    block_excl_scan<ST_THREADS, int32_t>(n, lds, &total);
    block_excl_scan<ST_THREADS, int32_t>(unm, lds, &nunm);
    block_excl_scan<ST_THREADS, int32_t>(bad_pos, lds, &npos);
    if (threadIdx.x == 0) {
        a.chunk_cnt[k] = total;
        m.chunk_unm[k] = nunm;
        a.chunk_bad[k] = (!ordered || npos) ? BAD_ORDER : BAD_NONE;
    }
}

// one block per chunk, under status PV_OK only: the rewrite. In place, rows that keep their label are not stored.
__global__ __launch_bounds__(ST_THREADS) void k_mask_write(StitchArgs a, MaskArgs m) {
    if (a.counts[1] != PV_OK) return;
    const int64_t k = blockIdx.x;
    const int32_t g = a.region[k];
    const int64_t rs = a.rstart[g], o0 = m.ref_off[g], span = m.ref_off[g + 1] - o0;
    const int64_t base = k * a.L;
    const bool lab_copy = m.lab_out != a.lab, qual_copy = m.qual_out != m.qual;
    for (int j = threadIdx.x; j < a.L; j += ST_THREADS) {
        const int64_t t = base + j;
        const int r = masked_label(a, m, t, rs, m.ref + o0, span);   // (status OK: no ROW_BAD_POS can come back)
        if (r >= 0) {
            m.lab_out[t] = (uint8_t)r;
            if (m.qual_out) m.qual_out[t] = 0;
        } else {
            if (lab_copy) m.lab_out[t] = a.lab[t];
            if (m.qual_out && qual_copy) m.qual_out[t] = m.qual[t];
        }
    }
}

}  // namespace

extern "C" int pv_polish_mask_low_depth_dev(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const uint8_t* labels,
                                            const uint8_t* row_qual, const int64_t* region_start, const int64_t* ref_off,
                                            const uint8_t* ref, int32_t n_regions, int seq_length, int min_depth, uint8_t* labels_out,
                                            uint8_t* row_qual_out, int64_t* d_counts, void* stream) {
    PV_CHECK(ctx && chunks && d_counts, PV_ERR_INVALID, "null argument");
    PV_CHECK(n_chunks >= 0 && n_regions >= 0 && seq_length >= 1, PV_ERR_INVALID, "negative sizes");
    PV_CHECK(min_depth >= 0 && min_depth <= 65535, PV_ERR_INVALID, "mask: min_depth %d is outside 0..65535", min_depth);
    PV_CHECK(chunks->depth, PV_ERR_INVALID, "mask: the chunks carry no depth plane (pv_polish_out.depth is null)");
    PV_CHECK(n_chunks <= chunks->chunk_capacity, PV_ERR_INVALID, "n_chunks %lld exceeds the chunk capacity %lld",
             (long long)n_chunks, (long long)chunks->chunk_capacity);
    PV_CHECK(n_chunks < (1ll << 31), PV_ERR_LIMIT, "too many chunks for one launch");
    PV_CHECK(n_chunks == 0 || ref, PV_ERR_INVALID, "mask: the batch carries no draft bytes (ref is null)");
    PV_CHECK(n_chunks == 0 || (chunks->position && chunks->index && chunks->region && chunks->chunk_id && labels && labels_out &&
                               region_start && ref_off && n_regions > 0),
             PV_ERR_INVALID, "chunk arrays, labels, region starts or draft offsets missing");
    PV_CHECK((row_qual != nullptr) == (row_qual_out != nullptr), PV_ERR_INVALID, "mask: row_qual and row_qual_out go together");
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = pv_pick_stream(ctx, stream);
    StitchArgs a = chunk_args(chunks, labels, region_start, n_chunks, n_regions, seq_length, 0, d_counts);
    MaskArgs m = {chunks->depth, row_qual, ref_off, ref, labels_out, row_qual_out, min_depth, nullptr};
    const size_t nk = (size_t)(n_chunks > 0 ? n_chunks : 1);
    int rc;
    if ((rc = pv_get(ctx, "mask.cnt", nk, &a.chunk_cnt))) return rc;
    if ((rc = pv_get(ctx, "mask.bad", nk, &a.chunk_bad))) return rc;
    if ((rc = pv_get(ctx, "mask.unm", nk, &m.chunk_unm))) return rc;
    pv_prof_scope ps_all(ctx, "polish_mask", st);
    if (n_chunks > 0) { pv_prof_scope ps(ctx, "k_mask_count", st); k_mask_count<<<(unsigned)n_chunks, ST_THREADS, 0, st>>>(a, m); }
    k_chunk_finish<<<1, ST_FINISH_THREADS, 0, st>>>(a, m.chunk_unm);
    if (n_chunks > 0) { pv_prof_scope ps(ctx, "k_mask_write", st); k_mask_write<<<(unsigned)n_chunks, ST_THREADS, 0, st>>>(a, m); }
    PV_HIP(hipGetLastError());
    return PV_OK;
}

extern "C" int pv_polish_mask_low_depth(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const uint8_t* labels,
                                        const uint8_t* row_qual, const int64_t* region_start, const int64_t* ref_off, const uint8_t* ref,
                                        int32_t n_regions, int seq_length, int min_depth, uint8_t* labels_out, uint8_t* row_qual_out,
                                        int64_t* counts) {
    PV_CHECK(ctx && chunks && counts, PV_ERR_INVALID, "null argument");
    PV_CHECK(n_chunks >= 0 && n_regions >= 0 && seq_length >= 1, PV_ERR_INVALID, "negative sizes");
    PV_CHECK(chunks->depth, PV_ERR_INVALID, "mask: the chunks carry no depth plane (pv_polish_out.depth is null)");
    PV_CHECK(n_chunks == 0 || (ref_off && n_regions > 0), PV_ERR_INVALID, "draft offsets missing");
    PV_CHECK(n_chunks == 0 || ref, PV_ERR_INVALID, "mask: the batch carries no draft bytes (ref is null)");
    PV_CHECK(n_chunks == 0 || (labels && labels_out), PV_ERR_INVALID, "labels missing");
    PV_CHECK((row_qual != nullptr) == (row_qual_out != nullptr), PV_ERR_INVALID, "mask: row_qual and row_qual_out go together");
    PV_CHECK(!ref_off || ref_off[n_regions] >= 0, PV_ERR_INVALID, "negative draft length");
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t nc = (size_t)n_chunks, L = (size_t)seq_length;
    pv_polish_out d;
    uint8_t *d_lab = nullptr, *d_rq = nullptr, *d_ref = nullptr, *d_lab_out = nullptr, *d_rq_out = nullptr;
    int64_t *d_rs = nullptr, *d_ro = nullptr, *d_counts = nullptr;
    int rc;
    if (row_qual && (rc = stage(ctx, "mk.row_qual", row_qual, nc * L, &d_rq, st))) return rc;
    if ((rc = stage_chunks(ctx, "mk", chunks, nc, L, true, false, &d, st))) return rc;
    if ((rc = stage(ctx, "mk.labels", labels, nc * L, &d_lab, st))) return rc;
    if ((rc = stage_draft(ctx, "mk", region_start, ref_off, ref, n_regions, &d_rs, &d_ro, &d_ref, st))) return rc;
    // in place on the host is in place on the device
    d_lab_out = d_lab;
    if (labels_out != labels && (rc = pv_get(ctx, "mk.labels_out", nc * L > 0 ? nc * L : 1, &d_lab_out))) return rc;
    d_rq_out = d_rq;
    if (row_qual && row_qual_out != row_qual && (rc = pv_get(ctx, "mk.row_qual_out", nc * L > 0 ? nc * L : 1, &d_rq_out))) return rc;
    if ((rc = pv_get(ctx, "mk.counts", (size_t)4, &d_counts))) return rc;
    rc = pv_polish_mask_low_depth_dev(ctx, &d, n_chunks, d_lab, row_qual ? d_rq : nullptr, d_rs, d_ro, d_ref, n_regions, seq_length,
                                      min_depth, d_lab_out, row_qual ? d_rq_out : nullptr, d_counts, st);
    if (rc) return rc;
    PV_HIP(hipMemcpyAsync(counts, d_counts, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    PV_HIP(hipStreamSynchronize(st));
    const int64_t status = counts[1];
    PV_CHECK(status != PV_ERR_INVALID, PV_ERR_INVALID,
             "mask: chunk %lld breaks the layout (regions ascending, chunk ids 0,1,2,... inside a region, masked positions inside "
             "the region's draft bytes)", (long long)counts[2]);
    PV_CHECK(status == PV_OK, (int)status, "mask: device status %lld", (long long)status);
    if (nc * L > 0) {
        PV_HIP(hipMemcpyAsync(labels_out, d_lab_out, nc * L, hipMemcpyDeviceToHost, st));
        if (row_qual) PV_HIP(hipMemcpyAsync(row_qual_out, d_rq_out, nc * L, hipMemcpyDeviceToHost, st));
        PV_HIP(hipStreamSynchronize(st));
    }
    return PV_OK;
}
