// polish_edits.hip — what the polisher changed in the draft: P2 labels + draft bytes -> one 16-byte record per edited column.
//
// The rule is in include/pepper_hip.h (pv_polish_edits). A column is kept and owned under the stitch's rules
// (polish_stitch.hip: the padding and the 200-position buffer are dropped, a (position, index) two chunks share belongs to
// the chunk whose id is last in decimal string order), with ownership decided before the label is looked at, so the owned
// columns are exactly those whose label the stitch consults. An owned index-0 column is compared with the draft byte under
// it; an owned insert column with a base label is an inserted base. Owned columns in chunk-major order are in
// (position, index) order, so ranking a chunk's edits behind the edits of the chunks before it gives the sorted list.
//
// Three launches as in the stitch, no global atomics: per-chunk counts (one block per chunk), the stitch's one-block scan of
// the counts into chunk offsets, region offsets and status, then a block-local scan per chunk and one 16-byte store per edit.
//
// pv_polish_edits_evidence is the same call with the write kernel's evidence twin: beside every record, one 8-byte record of
// the reads behind the edit (pv_polish_evidence), from the builder's depth and counts planes at the edit's own column.
#include "polish_stitch_common.hpp"

using namespace pv_chunks;

static_assert(sizeof(pv_polish_edit) == 16, "a record leaves as one 16-byte store");
static_assert(sizeof(pv_polish_evidence) == 8, "an evidence record leaves as one 8-byte store");

namespace {

// one block per chunk: edits the chunk contributes, and whether it breaks the layout (an owned position outside the region's
// draft counts as that: BAD_ORDER -> PV_ERR_INVALID) or holds a poisoned label on an owned column
__global__ __launch_bounds__(ST_THREADS) void k_edit_count(StitchArgs a, EditRefs r) {
    __shared__ int32_t lds[ST_THREADS / 64];
    const int64_t k = blockIdx.x;
    const bool ordered = chunk_in_order(a, k);
    int n = 0, bad_label = 0, bad_pos = 0;
    if (ordered) {
        const ChunkView v = chunk_view(a, k);
        const int32_t g = a.region[k];
        const int64_t o0 = r.ref_off[g], span = r.ref_off[g + 1] - o0;
        const int j0 = threadIdx.x * a.cpt, j1 = min(a.L, j0 + a.cpt);
        for (int j = j0; j < j1; j++) {
            const int32_t e = column_edit(a, r, v, r.ref + o0, span, j);
            n += is_edit(e);
            bad_label |= e == COL_BAD_LABEL;
            bad_pos |= e == COL_BAD_POS;
        }
    }
    int32_t total, nlabel, npos;
    block_excl_scan<ST_THREADS, int32_t>(n, lds, &total);
    block_excl_scan<ST_THREADS, int32_t>(bad_label, lds, &nlabel);
    block_excl_scan<ST_THREADS, int32_t>(bad_pos, lds, &npos);
    if (threadIdx.x == 0) {
        a.chunk_cnt[k] = total;
        a.chunk_bad[k] = (!ordered || npos) ? BAD_ORDER : (nlabel ? BAD_LABEL : BAD_NONE);
    }
}

// what the evidence twin of the write kernel reads and writes beside the records
struct EvRefs {
    const uint16_t* depth;    // chunks->depth
    const uint16_t* counts;   // chunks->counts, [row][10]
    pv_polish_evidence* ev;
};

__device__ __forceinline__ uint32_t halves(uint32_t x) { return (x & 0xFFFFu) + (x >> 16); }

// the evidence record of the edit `e` (column_edit's word) at chunk row t, as its two dwords (the rule is in pepper_hip.h;
// the reads behind the edit are edit_alt_counts, which the minimum-support filter shares)
__device__ __forceinline__ uint2 edit_evidence(const EvRefs& x, int64_t t, int32_t e) {
    const CountsRow w = counts_row(x.counts, t);
    const uint32_t depth = x.depth[t];
    const uint32_t kind = (uint32_t)e & 0xFF, d = ((uint32_t)e >> 8) & 0xFF;
    const uint2 alt = edit_alt_counts(w, e);
    const uint32_t fwd = alt.x, rev = alt.y;
    uint32_t ref;
    if (kind == PV_EDIT_INS) {
        const uint32_t sum = halves(w.w0) + halves(w.w1) + halves(w.w2) + halves(w.w3) + halves(w.w4);
        ref = depth > sum ? depth - sum : 0;
    } else {
        const uint32_t k = acgt_index(d >= 'a' && d <= 'z' ? d - 32 : d);
        ref = k < 4 ? row_count(w, k) + row_count(w, 4 + k) : 0;
    }
    if (ref > 65535u) ref = 65535u;
    return make_uint2(depth | ref << 16, fwd | rev << 16);
}

// one block per chunk: block-local ranks of the chunk's edits, then one 16-byte store each. EV: also one 8-byte evidence
// record each, from the counts row and the depth of the edit's own column, loaded for edits only; the instantiation without
// is the kernel as it was (x is not touched)
template <bool EV>
__global__ __launch_bounds__(ST_THREADS) void k_edit_write(StitchArgs a, EditRefs r, pv_polish_edit* edits, EvRefs x) {
    __shared__ int32_t lds[ST_THREADS / 64];
    if (a.counts[1] != PV_OK) return;
    const int64_t k = blockIdx.x;
    const ChunkView v = chunk_view(a, k);
    const int32_t g = a.region[k];
    const int64_t o0 = r.ref_off[g], span = r.ref_off[g + 1] - o0;
    const int j0 = threadIdx.x * a.cpt, j1 = min(a.L, j0 + a.cpt);
    int32_t es[ST_MAX_CPT];
    int n = 0;
    for (int j = j0; j < j1; j++) {
        const int32_t e = column_edit(a, r, v, r.ref + o0, span, j);   // (status OK: no COL_BAD code can come back)
        es[j - j0] = e;
        n += is_edit(e);
    }
    int32_t total;
    const int32_t r0 = block_excl_scan<ST_THREADS, int32_t>(n, lds, &total);
    uint4* dst = reinterpret_cast<uint4*>(edits + a.chunk_off[k] + r0);
    uint2* evd = EV ? reinterpret_cast<uint2*>(x.ev + a.chunk_off[k] + r0) : nullptr;
    for (int j = 0; j < j1 - j0; j++)
        if (is_edit(es[j])) {
            const int64_t t = v.base + j0 + j;
            const uint64_t p = (uint64_t)a.pos[t];
            *dst++ = make_uint4((uint32_t)p, (uint32_t)(p >> 32), (uint32_t)a.idx[t], (uint32_t)es[j]);
            if (EV) *evd++ = edit_evidence(x, t, es[j]);
        }
}

}  // namespace

// both device forms: want_ev picks the evidence twin of the write kernel (and checks what it reads and writes)
static int edits_launch(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const uint8_t* labels,
                        const uint8_t* row_qual, const int64_t* region_start, const int64_t* ref_off, const uint8_t* ref,
                        int32_t n_regions, int seq_length, int seq_overlap, int64_t* region_edit_off, pv_polish_edit* edits,
                        int64_t edit_capacity, int64_t* d_counts, void* stream, bool want_ev, pv_polish_evidence* evidence) {
    PV_CHECK(ctx && chunks && region_edit_off && d_counts, PV_ERR_INVALID, "null argument");
    PV_CHECK(n_chunks >= 0 && n_regions >= 0 && edit_capacity >= 0, PV_ERR_INVALID, "negative sizes");
    PV_CHECK(seq_length >= 1 && seq_length <= ST_THREADS * ST_MAX_CPT && seq_overlap >= 0 && seq_overlap < seq_length,
             PV_ERR_INVALID, "edits: need 1 <= seq_length <= %d and 0 <= seq_overlap < seq_length (got %d, %d)",
             ST_THREADS * ST_MAX_CPT, seq_length, seq_overlap);
    PV_CHECK(2 * seq_overlap <= seq_length, PV_ERR_INVALID, "edits: a column may overlap one neighbour chunk only (overlap %d)",
             seq_overlap);
    PV_CHECK(n_chunks <= chunks->chunk_capacity, PV_ERR_INVALID, "n_chunks %lld exceeds the chunk capacity %lld",
             (long long)n_chunks, (long long)chunks->chunk_capacity);
    PV_CHECK(n_chunks < (1ll << 31), PV_ERR_LIMIT, "too many chunks for one launch");
    PV_CHECK(n_chunks == 0 || (chunks->position && chunks->index && chunks->region && chunks->chunk_id && labels &&
                               region_start && ref_off && n_regions > 0),
             PV_ERR_INVALID, "chunk arrays, labels, region starts or draft offsets missing");
    PV_CHECK(n_chunks == 0 || ref, PV_ERR_INVALID, "edits: the batch carries no draft bytes (ref is null)");
    PV_CHECK(edit_capacity == 0 || edits, PV_ERR_INVALID, "edits missing");
    PV_CHECK(((uintptr_t)edits & 15) == 0, PV_ERR_INVALID, "edits is not aligned to 16 bytes");
    if (want_ev) {
        PV_CHECK(n_chunks == 0 || (chunks->depth && chunks->counts), PV_ERR_INVALID,
                 "evidence: the chunks carry no depth plane or no counts plane (pv_polish_out.depth, .counts)");
        PV_CHECK(edit_capacity == 0 || evidence, PV_ERR_INVALID, "evidence missing");
        PV_CHECK(((uintptr_t)evidence & 7) == 0, PV_ERR_INVALID, "evidence is not aligned to 8 bytes");
        PV_CHECK(((uintptr_t)chunks->counts & 3) == 0, PV_ERR_INVALID, "counts is not aligned to 4 bytes");
    }
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = pv_pick_stream(ctx, stream);
    StitchArgs a = chunk_args(chunks, labels, region_start, n_chunks, n_regions, seq_length, seq_overlap, d_counts);
    a.region_off = region_edit_off; a.cap = edit_capacity;
    EditRefs r = {ref_off, ref, row_qual};
    const size_t nk = (size_t)(n_chunks > 0 ? n_chunks : 1);
    int rc;
    if ((rc = pv_get(ctx, "edits.cnt", nk, &a.chunk_cnt))) return rc;
    if ((rc = pv_get(ctx, "edits.bad", nk, &a.chunk_bad))) return rc;
    if ((rc = pv_get(ctx, "edits.off", nk, &a.chunk_off))) return rc;
    const EvRefs x = {chunks->depth, chunks->counts, evidence};
    pv_prof_scope ps_all(ctx, want_ev ? "polish_edits_evidence" : "polish_edits", st);
    if (n_chunks > 0) { pv_prof_scope ps(ctx, "k_edit_count", st); k_edit_count<<<(unsigned)n_chunks, ST_THREADS, 0, st>>>(a, r); }
    k_stitch_scan<<<1, ST_SCAN_THREADS, 0, st>>>(a);
    if (n_chunks > 0) {
        pv_prof_scope ps(ctx, "k_edit_write", st);
        if (want_ev) k_edit_write<true><<<(unsigned)n_chunks, ST_THREADS, 0, st>>>(a, r, edits, x);
        else k_edit_write<false><<<(unsigned)n_chunks, ST_THREADS, 0, st>>>(a, r, edits, EvRefs{nullptr, nullptr, nullptr});
    }
    PV_HIP(hipGetLastError());
    return PV_OK;
}

extern "C" int pv_polish_edits_dev(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const uint8_t* labels,
                                   const uint8_t* row_qual, const int64_t* region_start, const int64_t* ref_off, const uint8_t* ref,
                                   int32_t n_regions, int seq_length, int seq_overlap, int64_t* region_edit_off, pv_polish_edit* edits,
                                   int64_t edit_capacity, int64_t* d_counts, void* stream) {
    return edits_launch(ctx, chunks, n_chunks, labels, row_qual, region_start, ref_off, ref, n_regions, seq_length, seq_overlap,
                        region_edit_off, edits, edit_capacity, d_counts, stream, false, nullptr);
}

extern "C" int pv_polish_edits_evidence_dev(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const uint8_t* labels,
                                            const uint8_t* row_qual, const int64_t* region_start, const int64_t* ref_off,
                                            const uint8_t* ref, int32_t n_regions, int seq_length, int seq_overlap,
                                            int64_t* region_edit_off, pv_polish_edit* edits, pv_polish_evidence* evidence,
                                            int64_t edit_capacity, int64_t* d_counts, void* stream) {
    return edits_launch(ctx, chunks, n_chunks, labels, row_qual, region_start, ref_off, ref, n_regions, seq_length, seq_overlap,
                        region_edit_off, edits, edit_capacity, d_counts, stream, true, evidence);
}

// both host forms
static int edits_host(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const uint8_t* labels,
                      const uint8_t* row_qual, const int64_t* region_start, const int64_t* ref_off, const uint8_t* ref,
                      int32_t n_regions, int seq_length, int seq_overlap, int64_t* region_edit_off, pv_polish_edit* edits,
                      int64_t edit_capacity, int64_t* counts, bool want_ev, pv_polish_evidence* evidence) {
    PV_CHECK(ctx && chunks && region_edit_off && counts, PV_ERR_INVALID, "null argument");
    PV_CHECK(n_chunks >= 0 && n_regions >= 0 && edit_capacity >= 0 && seq_length >= 1, PV_ERR_INVALID, "negative sizes");
    PV_CHECK(n_chunks == 0 || (ref_off && n_regions > 0), PV_ERR_INVALID, "draft offsets missing");
    PV_CHECK(n_chunks == 0 || ref, PV_ERR_INVALID, "edits: the batch carries no draft bytes (ref is null)");
    PV_CHECK(edit_capacity == 0 || edits, PV_ERR_INVALID, "edits missing");
    PV_CHECK(!ref_off || ref_off[n_regions] >= 0, PV_ERR_INVALID, "negative draft length");
    if (want_ev) {
        PV_CHECK(n_chunks == 0 || (chunks->depth && chunks->counts), PV_ERR_INVALID,
                 "evidence: the chunks carry no depth plane or no counts plane (pv_polish_out.depth, .counts)");
        PV_CHECK(edit_capacity == 0 || evidence, PV_ERR_INVALID, "evidence missing");
        PV_CHECK(((uintptr_t)evidence & 7) == 0, PV_ERR_INVALID, "evidence is not aligned to 8 bytes");
    }
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t nc = (size_t)n_chunks, L = (size_t)seq_length;
    pv_polish_out d;
    uint8_t *d_lab = nullptr, *d_rq = nullptr, *d_ref = nullptr;
    int64_t *d_rs = nullptr, *d_ro = nullptr, *d_eoff = nullptr, *d_counts = nullptr;
    pv_polish_edit* d_edits = nullptr;
    int rc;
    if (row_qual && (rc = stage(ctx, "ed.row_qual", row_qual, nc * L, &d_rq, st))) return rc;
    if ((rc = stage_chunks(ctx, "ed", chunks, nc, L, want_ev, want_ev, &d, st))) return rc;
    if ((rc = stage(ctx, "ed.labels", labels, nc * L, &d_lab, st))) return rc;
    if ((rc = stage_draft(ctx, "ed", region_start, ref_off, ref, n_regions, &d_rs, &d_ro, &d_ref, st))) return rc;
    if ((rc = pv_get(ctx, "ed.region_edit_off", (size_t)n_regions + 1, &d_eoff))) return rc;
    if ((rc = pv_get(ctx, "ed.edits", (size_t)(edit_capacity > 0 ? edit_capacity : 1), &d_edits))) return rc;
    if ((rc = pv_get(ctx, "ed.counts", (size_t)4, &d_counts))) return rc;
    pv_polish_evidence* d_ev = nullptr;
    if (want_ev && (rc = pv_get(ctx, "ed.evidence", (size_t)(edit_capacity > 0 ? edit_capacity : 1), &d_ev))) return rc;
    rc = edits_launch(ctx, &d, n_chunks, d_lab, row_qual ? d_rq : nullptr, d_rs, d_ro, d_ref, n_regions, seq_length, seq_overlap,
                      d_eoff, d_edits, edit_capacity, d_counts, st, want_ev, d_ev);
    if (rc) return rc;
    PV_HIP(hipMemcpyAsync(counts, d_counts, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    PV_HIP(hipMemcpyAsync(region_edit_off, d_eoff, ((size_t)n_regions + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    PV_HIP(hipStreamSynchronize(st));
    const int64_t status = counts[1];
    if (status == PV_ERR_CAPACITY) {
        pv_set_error("edits: capacity too small: need %lld records", (long long)counts[0]);
        return PV_ERR_CAPACITY;
    }
    PV_CHECK(status != PV_ERR_STATE, PV_ERR_STATE, "edits: chunk %lld holds a label outside 0..4 (a poisoned network result)",
             (long long)counts[2]);
    PV_CHECK(status != PV_ERR_INVALID, PV_ERR_INVALID,
             "edits: chunk %lld breaks the layout (regions ascending, chunk ids 0,1,2,... inside a region, positions inside the "
             "region's draft bytes)", (long long)counts[2]);
    PV_CHECK(status == PV_OK, (int)status, "edits: device status %lld", (long long)status);
    if (counts[0] > 0) {
        PV_HIP(hipMemcpyAsync(edits, d_edits, (size_t)counts[0] * sizeof(pv_polish_edit), hipMemcpyDeviceToHost, st));
        if (want_ev)
            PV_HIP(hipMemcpyAsync(evidence, d_ev, (size_t)counts[0] * sizeof(pv_polish_evidence), hipMemcpyDeviceToHost, st));
        PV_HIP(hipStreamSynchronize(st));
    }
    return PV_OK;
}

extern "C" int pv_polish_edits(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const uint8_t* labels,
                               const uint8_t* row_qual, const int64_t* region_start, const int64_t* ref_off, const uint8_t* ref,
                               int32_t n_regions, int seq_length, int seq_overlap, int64_t* region_edit_off, pv_polish_edit* edits,
                               int64_t edit_capacity, int64_t* counts) {
    return edits_host(ctx, chunks, n_chunks, labels, row_qual, region_start, ref_off, ref, n_regions, seq_length, seq_overlap,
                      region_edit_off, edits, edit_capacity, counts, false, nullptr);
}

extern "C" int pv_polish_edits_evidence(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const uint8_t* labels,
                                        const uint8_t* row_qual, const int64_t* region_start, const int64_t* ref_off,
                                        const uint8_t* ref, int32_t n_regions, int seq_length, int seq_overlap,
                                        int64_t* region_edit_off, pv_polish_edit* edits, pv_polish_evidence* evidence,
                                        int64_t edit_capacity, int64_t* counts) {
    return edits_host(ctx, chunks, n_chunks, labels, row_qual, region_start, ref_off, ref, n_regions, seq_length, seq_overlap,
                      region_edit_off, edits, edit_capacity, counts, true, evidence);
}
