// polish_stitch.hip — the polisher's stitch step (P2 labels -> polished bases) on the device.
//
// Restates pepper/modules/python/Stitch.py:37-86 (small_chunk_stitch) for the chunk batches that
// pv_polish_summarize_regions[_dev] writes and pv_rnn_forward_p2[_dev] labels:
//   * a column is dropped when index < 0 or position < 0 (padding), and when region_start > 0 and
//     position <= region_start + 2*MIN_IMAGE_OVERLAP (the overlap with the previous region);
//   * the (position, index) pairs shared by two chunks of a region (the seq_overlap columns) keep the label
//     of the chunk whose id is LAST IN STRING ORDER ("9" after "10"): the reference walks sorted() HDF5 key names;
//   * label 0 gives no base, 1..4 give A, C, G, T; any other kept label (255 = a poisoned P2 result) is an error.
// The builder's rows run in (position, index) order inside a region, so emitting the surviving columns in
// chunk-major order is the reference's sort, and the per-region results concatenated are its per-contig string.
//
// Three launches, no global atomics: per-chunk counts (one block per chunk), one block scanning the chunk counts
// into offsets (+ status, region offsets), then a block-local scan per chunk and a scattered byte write.
#include "polish_stitch_common.hpp"

using namespace pv_chunks;

namespace {

// 0: no base, 1..4: base, -1: a kept column with a label outside 0..4
__device__ inline int column_label(const StitchArgs& a, const ChunkView& v, int j) {
    const int64_t t = v.base + j;
    const int64_t p = a.pos[t];
    const int32_t x = a.idx[t];
    if (p < 0 || x < 0) return 0;
    if (v.rs > 0 && p <= v.rs + ST_BUFFER) return 0;
    const int lb = a.lab[t];
    if (lb > 4) return -1;
    if (lb == 0) return 0;
    const int ov = a.L - a.step;
    if (v.prev && j < ov) {   // also column j + step of the previous chunk
        const int64_t u = t - a.L + a.step;
        if (a.pos[u] == p && a.idx[u] == x && !dec_str_gt(v.c, v.cprev)) return 0;
    }
    if (v.next && j >= a.step) {   // also column j - step of the next chunk
        const int64_t u = t + a.L - a.step;
        if (a.pos[u] == p && a.idx[u] == x && !dec_str_gt(v.c, v.cnext)) return 0;
    }
    return lb;
}

// one block per chunk: bases the chunk contributes, and whether it breaks the layout or holds a poisoned label
__global__ __launch_bounds__(ST_THREADS) void k_stitch_count(StitchArgs a) {
    __shared__ int32_t lds[ST_THREADS / 64];
    const int64_t k = blockIdx.x;
    const bool ordered = chunk_in_order(a, k);
    int n = 0, bad = 0;
    if (ordered) {
        const ChunkView v = chunk_view(a, k);
        const int j0 = threadIdx.x * a.cpt, j1 = min(a.L, j0 + a.cpt);
        for (int j = j0; j < j1; j++) {
            const int lb = column_label(a, v, j);
            n += lb > 0;
            bad |= lb < 0;
        }
    }
    int32_t total, nbad;
    block_excl_scan<ST_THREADS, int32_t>(n, lds, &total);
    block_excl_scan<ST_THREADS, int32_t>(bad, lds, &nbad);
    if (threadIdx.x == 0) {
        a.chunk_cnt[k] = total;
        a.chunk_bad[k] = !ordered ? BAD_ORDER : (nbad ? BAD_LABEL : BAD_NONE);
    }
}

// one block per chunk: block-local ranks of the emitted columns, then one byte each; QUAL: and the column's row quality
// (pv_polish_row_qual) into a second plane at the same offset
template <bool QUAL>
__global__ __launch_bounds__(ST_THREADS) void k_stitch_write(StitchArgs a, const uint8_t* row_qual, uint8_t* qual) {
    __shared__ int32_t lds[ST_THREADS / 64];
    if (a.counts[1] != PV_OK) return;
    const int64_t k = blockIdx.x;
    const ChunkView v = chunk_view(a, k);
    const int j0 = threadIdx.x * a.cpt, j1 = min(a.L, j0 + a.cpt);
    uint8_t lbs[ST_MAX_CPT];
    int n = 0;
    for (int j = j0; j < j1; j++) {
        const int lb = column_label(a, v, j);
        lbs[j - j0] = (uint8_t)(lb > 0 ? lb : 0);
        n += lb > 0;
    }
    int32_t total;
    const int32_t r0 = block_excl_scan<ST_THREADS, int32_t>(n, lds, &total);
    uint8_t* dst = a.seq + a.chunk_off[k] + r0;
    for (int j = 0; j < j1 - j0; j++)
        if (lbs[j]) *dst++ = "ACGT"[lbs[j] - 1];
    if (QUAL) {
        uint8_t* qdst = qual + a.chunk_off[k] + r0;
        const uint8_t* q = row_qual + v.base + j0;
        for (int j = 0; j < j1 - j0; j++)
            if (lbs[j]) *qdst++ = q[j];
    }
}

}  // namespace

// the device form of both stitches; QUAL: with the quality plane
template <bool QUAL>
static int stitch_dev(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const uint8_t* labels, const uint8_t* row_qual,
                      const int64_t* region_start, int32_t n_regions, int seq_length, int seq_overlap, int64_t* region_off,
                      uint8_t* seq, uint8_t* qual, int64_t seq_capacity, int64_t* d_counts, void* stream) {
    PV_CHECK(ctx && chunks && region_off && d_counts, PV_ERR_INVALID, "null argument");
    PV_CHECK(n_chunks >= 0 && n_regions >= 0 && seq_capacity >= 0, PV_ERR_INVALID, "negative sizes");
    PV_CHECK(seq_length >= 1 && seq_length <= ST_THREADS * ST_MAX_CPT && seq_overlap >= 0 && seq_overlap < seq_length,
             PV_ERR_INVALID, "stitch: need 1 <= seq_length <= %d and 0 <= seq_overlap < seq_length (got %d, %d)",
             ST_THREADS * ST_MAX_CPT, seq_length, seq_overlap);
    PV_CHECK(2 * seq_overlap <= seq_length, PV_ERR_INVALID, "stitch: a column may overlap one neighbour chunk only (overlap %d)",
             seq_overlap);
    PV_CHECK(n_chunks <= chunks->chunk_capacity, PV_ERR_INVALID, "n_chunks %lld exceeds the chunk capacity %lld",
             (long long)n_chunks, (long long)chunks->chunk_capacity);
    PV_CHECK(n_chunks < (1ll << 31), PV_ERR_LIMIT, "too many chunks for one launch");
    PV_CHECK(n_chunks == 0 || (chunks->position && chunks->index && chunks->region && chunks->chunk_id && labels &&
                               region_start && n_regions > 0),
             PV_ERR_INVALID, "chunk arrays, labels or region starts missing");
    PV_CHECK(seq_capacity == 0 || seq, PV_ERR_INVALID, "seq missing");
    if (QUAL) PV_CHECK((n_chunks == 0 || row_qual) && (seq_capacity == 0 || qual), PV_ERR_INVALID, "row_qual or qual missing");
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = pv_pick_stream(ctx, stream);
    StitchArgs a = chunk_args(chunks, labels, region_start, n_chunks, n_regions, seq_length, seq_overlap, d_counts);
    a.region_off = region_off; a.seq = seq; a.cap = seq_capacity;
    const size_t nk = (size_t)(n_chunks > 0 ? n_chunks : 1);
    int rc;
    if ((rc = pv_get(ctx, "stitch.cnt", nk, &a.chunk_cnt))) return rc;
    if ((rc = pv_get(ctx, "stitch.bad", nk, &a.chunk_bad))) return rc;
    if ((rc = pv_get(ctx, "stitch.off", nk, &a.chunk_off))) return rc;
    pv_prof_scope ps_all(ctx, "polish_stitch", st);
    if (n_chunks > 0) { pv_prof_scope ps(ctx, "k_stitch_count", st); k_stitch_count<<<(unsigned)n_chunks, ST_THREADS, 0, st>>>(a); }
    k_stitch_scan<<<1, ST_SCAN_THREADS, 0, st>>>(a);
    if (n_chunks > 0) {
        pv_prof_scope ps(ctx, QUAL ? "k_stitch_write_qual" : "k_stitch_write", st);
        k_stitch_write<QUAL><<<(unsigned)n_chunks, ST_THREADS, 0, st>>>(a, row_qual, qual);
    }
    PV_HIP(hipGetLastError());
    return PV_OK;
}

extern "C" int pv_polish_stitch_dev(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const uint8_t* labels,
                                    const int64_t* region_start, int32_t n_regions, int seq_length, int seq_overlap,
                                    int64_t* region_off, uint8_t* seq, int64_t seq_capacity, int64_t* d_counts, void* stream) {
    return stitch_dev<false>(ctx, chunks, n_chunks, labels, nullptr, region_start, n_regions, seq_length, seq_overlap, region_off,
                             seq, nullptr, seq_capacity, d_counts, stream);
}

extern "C" int pv_polish_stitch_qual_dev(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const uint8_t* labels,
                                         const int64_t* region_start, int32_t n_regions, int seq_length, int seq_overlap,
                                         int64_t* region_off, uint8_t* seq, int64_t seq_capacity, int64_t* d_counts, void* stream,
                                         const uint8_t* row_qual, uint8_t* qual) {
    return stitch_dev<true>(ctx, chunks, n_chunks, labels, row_qual, region_start, n_regions, seq_length, seq_overlap, region_off,
                            seq, qual, seq_capacity, d_counts, stream);
}

// the host form of both stitches; QUAL: with the quality plane
template <bool QUAL>
static int stitch_host(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const uint8_t* labels, const uint8_t* row_qual,
                       const int64_t* region_start, int32_t n_regions, int seq_length, int seq_overlap, int64_t* region_off,
                       uint8_t* seq, uint8_t* qual, int64_t seq_capacity, int64_t* counts) {
    PV_CHECK(ctx && chunks && region_off && counts, PV_ERR_INVALID, "null argument");
    if (QUAL) PV_CHECK((n_chunks == 0 || row_qual) && (seq_capacity == 0 || qual), PV_ERR_INVALID, "row_qual or qual missing");
    PV_CHECK(n_chunks >= 0 && n_regions >= 0 && seq_capacity >= 0 && seq_length >= 1, PV_ERR_INVALID, "negative sizes");
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t nc = (size_t)n_chunks, L = (size_t)seq_length;
    pv_polish_out d;
    const uint8_t* d_lab = nullptr;
    const int64_t* d_rs = nullptr;
    int64_t *d_roff = nullptr, *d_counts = nullptr;
    uint8_t *d_seq = nullptr, *d_qual = nullptr;
    const uint8_t* d_rq = nullptr;
    int rc;
    if (QUAL) {
        if ((rc = stage(ctx, "st.row_qual", row_qual, nc * L, (uint8_t**)&d_rq, st))) return rc;
        if ((rc = pv_get(ctx, "st.qual", (size_t)(seq_capacity > 0 ? seq_capacity : 1), &d_qual))) return rc;
    }
    if ((rc = stage_chunks(ctx, "st", chunks, nc, L, false, false, &d, st))) return rc;
    if ((rc = stage(ctx, "st.labels", labels, nc * L, (uint8_t**)&d_lab, st))) return rc;
    if ((rc = stage(ctx, "st.region_start", region_start, (size_t)n_regions, (int64_t**)&d_rs, st))) return rc;
    if ((rc = pv_get(ctx, "st.region_off", (size_t)n_regions + 1, &d_roff))) return rc;
    if ((rc = pv_get(ctx, "st.seq", (size_t)(seq_capacity > 0 ? seq_capacity : 1), &d_seq))) return rc;
    if ((rc = pv_get(ctx, "st.counts", (size_t)4, &d_counts))) return rc;
    rc = stitch_dev<QUAL>(ctx, &d, n_chunks, d_lab, d_rq, d_rs, n_regions, seq_length, seq_overlap, d_roff, d_seq, d_qual,
                          seq_capacity, d_counts, st);
    if (rc) return rc;
    PV_HIP(hipMemcpyAsync(counts, d_counts, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    PV_HIP(hipMemcpyAsync(region_off, d_roff, ((size_t)n_regions + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    PV_HIP(hipStreamSynchronize(st));
    const int64_t status = counts[1];
    if (status == PV_ERR_CAPACITY) {
        pv_set_error("stitch: seq capacity too small: need %lld bases", (long long)counts[0]);
        return PV_ERR_CAPACITY;
    }
    PV_CHECK(status != PV_ERR_STATE, PV_ERR_STATE, "stitch: chunk %lld holds a label outside 0..4 (a poisoned network result)",
             (long long)counts[2]);
    PV_CHECK(status != PV_ERR_INVALID, PV_ERR_INVALID,
             "stitch: chunk %lld breaks the layout (regions ascending, chunk ids 0,1,2,... inside a region)", (long long)counts[2]);
    PV_CHECK(status == PV_OK, (int)status, "stitch: device status %lld", (long long)status);
    if (counts[0] > 0) {
        PV_HIP(hipMemcpyAsync(seq, d_seq, (size_t)counts[0], hipMemcpyDeviceToHost, st));
        if (QUAL) PV_HIP(hipMemcpyAsync(qual, d_qual, (size_t)counts[0], hipMemcpyDeviceToHost, st));
        PV_HIP(hipStreamSynchronize(st));
    }
    return PV_OK;
}

extern "C" int pv_polish_stitch(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const uint8_t* labels,
                                const int64_t* region_start, int32_t n_regions, int seq_length, int seq_overlap,
                                int64_t* region_off, uint8_t* seq, int64_t seq_capacity, int64_t* counts) {
    return stitch_host<false>(ctx, chunks, n_chunks, labels, nullptr, region_start, n_regions, seq_length, seq_overlap, region_off,
                              seq, nullptr, seq_capacity, counts);
}

extern "C" int pv_polish_stitch_qual(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const uint8_t* labels,
                                     const int64_t* region_start, int32_t n_regions, int seq_length, int seq_overlap,
                                     int64_t* region_off, uint8_t* seq, int64_t seq_capacity, int64_t* counts,
                                     const uint8_t* row_qual, uint8_t* qual) {
    return stitch_host<true>(ctx, chunks, n_chunks, labels, row_qual, region_start, n_regions, seq_length, seq_overlap, region_off,
                             seq, qual, seq_capacity, counts);
}
