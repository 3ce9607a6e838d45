// summary_host.hip — the host-buffer entry points of the three summary builders: validate and upload a batch, launch with
// the workspace heuristics, launch again with larger ones when the device reports a limit, copy the results down. No
// kernels live here: the launches are those of summary_builder.hip and summary_polish.hip (summary_launch.hpp).
#include "batch_check.hpp"
#include "summary_launch.hpp"

using namespace pvsum;

// `bytes` of host memory -> the workspace slot `name` (asynchronous copy on `st`)
static int upload_bytes(pv_ctx* ctx, const char* name, const void* h, size_t bytes, size_t min_bytes, const void** d, hipStream_t st) {
    void* p = nullptr;
    int rc = ctx->arena.get(name, bytes ? bytes : min_bytes, &p);
    if (rc) return rc;
    if (bytes) PV_HIP(hipMemcpyAsync(p, h, bytes, hipMemcpyHostToDevice, st));
    *d = p;
    return PV_OK;
}

// Every array of the host batch `in` that `shape.reads` names (and every array no bit stands for) -> its workspace slot; `dev`
// receives the device pointers, null for the arrays left out.
static int upload_arrays(pv_ctx* ctx, const pv_batch_in* in, const pv_batch_shape& shape, pv_batch_in* dev, hipStream_t st) {
    dev->n_regions = in->n_regions;
    dev->reserved = in->reserved;
    for (const pv_batch_array& row : pv_batch_arrays) {
        const void** dst = reinterpret_cast<const void**>(reinterpret_cast<char*>(dev) + row.field);
        *dst = nullptr;
        if (row.bit && !(shape.reads & row.bit)) continue;
        const void* src = *reinterpret_cast<const void* const*>(reinterpret_cast<const char*>(in) + row.field);
        int rc = upload_bytes(ctx, row.slot, src, (size_t)(shape.*row.count + row.plus) * row.elem, row.elem, dst, st);
        if (rc) return rc;
    }
    return PV_OK;
}

// The verdict of pv_check_batch in the words of the entry point: pv_upload_batches names the part (part >= 0).
static int batch_error(const pv_batch_shape& s, int part) {
    char colon[32] = "", space[32] = "";   // "part 3: " and "part 3 "
    if (part >= 0) {
        snprintf(colon, sizeof(colon), "part %d: ", part);
        snprintf(space, sizeof(space), "part %d ", part);
    }
    switch (s.fault) {
        case PV_BF_REGION_COUNT:
            if (part >= 0) pv_set_error("part %d: bad region count", part);
            else pv_set_error("negative region count");
            break;
        case PV_BF_OFFSET_START: pv_set_error("%soffset arrays must start at 0", colon); break;
        case PV_BF_REGION_EMPTY:
        case PV_BF_REF_SHORT: pv_set_error("%sregion %d: reference shorter than ref_end-ref_start+1", space, (int)s.index); break;
        case PV_BF_READ_OFF: pv_set_error("read_off not monotone"); break;
        default: pv_set_error("%sread %lld: offsets not monotone", space, (long long)s.index); break;
    }
    return s.code;
}

// The arrays of a HOST batch -> the context's workspace (asynchronous copies on `stream`); `dev` receives the same struct with
// DEVICE pointers, valid until the next upload on this context. The offset arrays are validated on the host first (cheap:
// O(regions + reads)). totals4 = {n_reads, n_bases, n_cigar, n_ref_bytes}: what the *_dev entry points take next to the struct.
extern "C" int pv_upload_batch(pv_ctx* ctx, const pv_batch_in* in, pv_batch_in* dev, int64_t* totals4, void* stream) {
    PV_CHECK(ctx && in && dev && totals4, PV_ERR_INVALID, "null argument");
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = pv_pick_stream(ctx, stream);
    const pv_batch_shape shape = pv_check_batch(in, PV_BATCH_BUILDER);
    if (shape.code) return batch_error(shape, -1);
    *dev = *in;
    totals4[0] = shape.n_reads; totals4[1] = shape.n_bases; totals4[2] = shape.n_cigar; totals4[3] = shape.n_cols;
    if (in->n_regions == 0) return PV_OK;
    return upload_arrays(ctx, in, shape, dev, st);
}

// The same for a batch that arrives in PARTS (e.g. one part per interval from the reader threads): the parts are laid end to
// end on the device - the large arrays (reference, bases, qualities, CIGAR) are copied part by part straight to their offsets,
// only the small per-region / per-read arrays are rebased on the host - so the caller never concatenates ~15 MB per interval.
extern "C" int pv_upload_batches(pv_ctx* ctx, int n_parts, const pv_batch_in* const* parts, pv_batch_in* dev, int64_t* totals4, void* stream) {
    PV_CHECK(ctx && parts && dev && totals4 && n_parts >= 0, PV_ERR_INVALID, "null argument");
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = pv_pick_stream(ctx, stream);
    pv_batch_shape all = {PV_OK, PV_BF_NONE, -1, "ok", PV_BA_CANDS, 0, 0, 0, 0, 0};   // the small arrays go up from the staging below
    for (int k = 0; k < n_parts; k++) {
        PV_CHECK(parts[k], PV_ERR_INVALID, "part %d: bad region count", k);
        const pv_batch_shape s = pv_check_batch(parts[k], PV_BATCH_BUILDER);
        if (s.code) return batch_error(s, k);
        all.n_regions += parts[k]->n_regions;
        all.n_reads += s.n_reads; all.n_bases += s.n_bases; all.n_cigar += s.n_cigar; all.n_cols += s.n_cols;
    }
    const int64_t G = all.n_regions;
    PV_CHECK(G < (1ll << 31), PV_ERR_LIMIT, "too many regions");
    memset(dev, 0, sizeof(*dev));
    dev->n_regions = (int32_t)G;
    const int64_t n_reads = all.n_reads, n_bases = all.n_bases, n_cigar = all.n_cigar, n_cols = all.n_cols;
    totals4[0] = n_reads; totals4[1] = n_bases; totals4[2] = n_cigar; totals4[3] = n_cols;
    if (G == 0) return PV_OK;
    // small arrays: rebased on the host into one staging vector per array (kept alive in the context until the next upload)
    std::vector<int64_t>& hs = ctx->upload_i64;
    std::vector<uint8_t>& hb = ctx->upload_u8;
    const size_t n64 = (size_t)(4 * G + 2 * (G + 1) + n_reads + 2 * (n_reads + 1));
    hs.resize(n64);
    hb.resize((size_t)(2 * n_reads));
    int64_t* h_ref_start = hs.data(); int64_t* h_ref_end = h_ref_start + G; int64_t* h_cand_start = h_ref_end + G; int64_t* h_cand_end = h_cand_start + G;
    int64_t* h_ref_off = h_cand_end + G; int64_t* h_read_off = h_ref_off + (G + 1); int64_t* h_read_pos = h_read_off + (G + 1);
    int64_t* h_base_off = h_read_pos + n_reads; int64_t* h_cigar_off = h_base_off + (n_reads + 1);
    uint8_t* h_flags = hb.data(); uint8_t* h_mapq = h_flags + n_reads;
    uint8_t *d_ref = nullptr, *d_bases = nullptr, *d_quals = nullptr;
    uint32_t* d_cigar = nullptr;
    int rc;
    if ((rc = pv_get(ctx, "in.ref", (size_t)std::max<int64_t>(n_cols, 1), &d_ref)) || (rc = pv_get(ctx, "in.bases", (size_t)std::max<int64_t>(n_bases, 1), &d_bases)) ||
        (rc = pv_get(ctx, "in.quals", (size_t)std::max<int64_t>(n_bases, 1), &d_quals)) || (rc = pv_get(ctx, "in.cigar", (size_t)std::max<int64_t>(n_cigar, 1), &d_cigar)))
        return rc;
    int64_t g0 = 0, r0 = 0, b0 = 0, c0 = 0, col0 = 0;
    h_ref_off[0] = 0; h_read_off[0] = 0; h_base_off[0] = 0; h_cigar_off[0] = 0;
    for (int k = 0; k < n_parts; k++) {
        const pv_batch_in* in = parts[k];
        const int g = in->n_regions;
        if (g == 0) continue;
        const int64_t nr = in->read_off[g], nb = nr ? in->base_off[nr] : 0, nc = nr ? in->cigar_off[nr] : 0, ncol = in->ref_off[g];
        for (int i = 0; i < g; i++) {
            h_ref_start[g0 + i] = in->ref_start[i]; h_ref_end[g0 + i] = in->ref_end[i];
            h_cand_start[g0 + i] = in->cand_start[i]; h_cand_end[g0 + i] = in->cand_end[i];
            h_ref_off[g0 + i + 1] = col0 + in->ref_off[i + 1];
            h_read_off[g0 + i + 1] = r0 + in->read_off[i + 1];
        }
        for (int64_t r = 0; r < nr; r++) {
            h_read_pos[r0 + r] = in->read_pos[r];
            h_flags[r0 + r] = in->read_flags[r]; h_mapq[r0 + r] = in->read_mapq[r];
            h_base_off[r0 + r + 1] = b0 + in->base_off[r + 1];
            h_cigar_off[r0 + r + 1] = c0 + in->cigar_off[r + 1];
        }
        if (ncol) PV_HIP(hipMemcpyAsync(d_ref + col0, in->ref, (size_t)ncol, hipMemcpyHostToDevice, st));
        if (nb) {
            PV_HIP(hipMemcpyAsync(d_bases + b0, in->bases, (size_t)nb, hipMemcpyHostToDevice, st));
            PV_HIP(hipMemcpyAsync(d_quals + b0, in->quals, (size_t)nb, hipMemcpyHostToDevice, st));
        }
        if (nc) PV_HIP(hipMemcpyAsync(d_cigar + c0, in->cigar, (size_t)nc * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        g0 += g; r0 += nr; b0 += nb; c0 += nc; col0 += ncol;
    }
    pv_batch_in h;
    memset(&h, 0, sizeof(h));
    h.n_regions = (int32_t)G;
    h.ref_start = h_ref_start; h.ref_end = h_ref_end; h.cand_start = h_cand_start; h.cand_end = h_cand_end;
    h.ref_off = h_ref_off; h.read_off = h_read_off; h.read_pos = h_read_pos; h.read_flags = h_flags; h.read_mapq = h_mapq;
    h.base_off = h_base_off; h.cigar_off = h_cigar_off;
    if ((rc = upload_arrays(ctx, &h, all, dev, st))) return rc;
    dev->ref = d_ref; dev->bases = d_bases; dev->quals = d_quals; dev->cigar = d_cigar;
    return PV_OK;
}

// One host-form call behind its upload: launch(), read the four counters back, and - while the device reports PV_ERR_LIMIT, at
// most twice - enlarge(counters) the workspace limits and launch again. Then the device status in words; limit_msg (may be
// null) is what PV_ERR_LIMIT means for the caller. The counters are left in ctx->h_counts.
template <typename Launch, typename Enlarge>
static int launch_and_count(pv_ctx* ctx, const int64_t* d_counts, hipStream_t st, const char* limit_msg, Launch launch, Enlarge enlarge) {
    for (int attempt = 0; attempt < 3; attempt++) {
        int rc = launch();
        if (rc) return rc;
        PV_HIP(hipMemcpyAsync(ctx->h_counts, d_counts, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        PV_HIP(hipStreamSynchronize(st));
        if (ctx->h_counts[2] != PV_ERR_LIMIT || attempt == 2) break;
        enlarge(ctx->h_counts);
    }
    const int64_t status = ctx->h_counts[2];
    PV_CHECK(status != PV_ERR_INVALID, PV_ERR_INVALID, "malformed read: CIGAR walks past the end of its bases");
    if (limit_msg) PV_CHECK(status != PV_ERR_LIMIT, PV_ERR_LIMIT, "%s", limit_msg);
    PV_CHECK(status == 0, (int)status, "device status %lld", (long long)status);
    return PV_OK;
}

static int summarize_host(pv_ctx* ctx, const pv_batch_in* in, const pv_params* params, pv_batch_out* out, bool hp,
                          const int32_t* read_hp);
extern "C" int pv_summarize_regions(pv_ctx* ctx, const pv_batch_in* in, const pv_params* params, pv_batch_out* out) {
    return summarize_host(ctx, in, params, out, false, nullptr);
}
extern "C" int pv_summarize_regions_hp(pv_ctx* ctx, const pv_batch_in* in, const int32_t* read_hp, const pv_params* params,
                                       pv_batch_out* out) {
    return summarize_host(ctx, in, params, out, true, read_hp);
}

// host buffers in and out; `hp` selects the haplotag-aware builder (window bytes, one more input array)
static int summarize_host(pv_ctx* ctx, const pv_batch_in* in, const pv_params* params, pv_batch_out* out, bool hp,
                          const int32_t* read_hp) {
    PV_CHECK(ctx && in && params && out, PV_ERR_INVALID, "null argument");
    const size_t WB = hp ? PV_HP_WINDOW_BYTES : PV_WINDOW_BYTES;
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int G = in->n_regions;
    out->n_out = 0;
    out->str_bytes = 0;
    if (out->capacity > 0 && out->cand_off) out->cand_off[0] = 0;
    if (G <= 0) return PV_OK;
    for (int g = 0; g < G; g++)
        PV_CHECK(in->read_off[g + 1] - in->read_off[g] <= MAX_REGION_READS, PV_ERR_LIMIT,
                 "region %d holds %lld reads: the counter planes are 16-bit (at most %d reads per region; the reference's caller "
                 "down-samples to 5000)", g, (long long)(in->read_off[g + 1] - in->read_off[g]), MAX_REGION_READS);
    pv_batch_in d;
    int64_t totals[4];
    int rc = pv_upload_batch(ctx, in, &d, totals, st);
    if (rc) return rc;
    const int64_t n_reads = totals[0], n_bases = totals[1], n_cigar = totals[2], n_cols = totals[3];
    const void* d_hp = nullptr;
    if (hp && read_hp)
        if ((rc = upload_bytes(ctx, "in.read_hp", read_hp, (size_t)n_reads * sizeof(int32_t), sizeof(int32_t), &d_hp, st))) return rc;

    const int64_t cap = out->capacity > 0 ? out->capacity : 0, scap = out->str_capacity > 0 ? out->str_capacity : 0;
    pv_batch_out dout = *out;
    if ((rc = pv_get(ctx, "out.region", cap + 1, &dout.region))) return rc;
    if ((rc = pv_get(ctx, "out.position", cap + 1, &dout.position))) return rc;
    if ((rc = pv_get(ctx, "out.depth", cap + 1, &dout.depth))) return rc;
    if ((rc = pv_get(ctx, "out.cand_freq", cap + 1, &dout.cand_freq))) return rc;
    if ((rc = pv_get(ctx, "out.images", (size_t)(cap + 1) * WB, &dout.images))) return rc;
    dout.images_i32 = nullptr;
    if (out->images_i32)
        if ((rc = pv_get(ctx, "out.images_i32", (size_t)(cap + 1) * WB, &dout.images_i32))) return rc;
    if ((rc = pv_get(ctx, "out.cand_str", scap + 1, &dout.cand_str))) return rc;
    if ((rc = pv_get(ctx, "out.cand_off", cap + 2, &dout.cand_off))) return rc;
    int64_t* d_counts = nullptr;
    if ((rc = pv_get(ctx, "out.counts", (size_t)4, &d_counts))) return rc;

    // workspace heuristics first; when they prove too small, exact bounds
    int64_t ms, me, mp;
    default_limits(n_cols, n_cigar, n_bases, n_reads, cap, hp, &ms, &me, &mp);
    char limit_msg[96];
    snprintf(limit_msg, sizeof(limit_msg), "more than %d distinct alleles at one site, or index range exceeded", UMAX);
    rc = launch_and_count(
        ctx, d_counts, st, limit_msg,
        [&] { return summarize_launch(ctx, &d, params, n_reads, n_bases, n_cigar, n_cols, ms, me, mp, &dout, d_counts, st, hp, (const int32_t*)d_hp); },
        [&](const int64_t*) {
            ms = n_cols;
            me = n_cigar + n_bases;
            mp = n_reads * ((n_cols + TILE_COLS - 1) / TILE_COLS + 2);
        });
    if (rc) return rc;
    out->n_out = ctx->h_counts[0];
    out->str_bytes = ctx->h_counts[1];
    if (out->n_out > cap || out->str_bytes > scap) {
        pv_set_error("output capacity too small: need %lld windows, %lld key bytes", (long long)out->n_out,
                     (long long)out->str_bytes);
        return PV_ERR_CAPACITY;
    }
    const int64_t n = out->n_out;
    if (n > 0) {
        PV_HIP(hipMemcpyAsync(out->region, dout.region, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        PV_HIP(hipMemcpyAsync(out->position, dout.position, n * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        PV_HIP(hipMemcpyAsync(out->depth, dout.depth, n, hipMemcpyDeviceToHost, st));
        PV_HIP(hipMemcpyAsync(out->cand_freq, dout.cand_freq, n, hipMemcpyDeviceToHost, st));
        PV_HIP(hipMemcpyAsync(out->images, dout.images, n * WB, hipMemcpyDeviceToHost, st));
        if (out->images_i32)
            PV_HIP(hipMemcpyAsync(out->images_i32, dout.images_i32, n * WB * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        PV_HIP(hipMemcpyAsync(out->cand_str, dout.cand_str, out->str_bytes, hipMemcpyDeviceToHost, st));
        PV_HIP(hipMemcpyAsync(out->cand_off, dout.cand_off, (n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        PV_HIP(hipStreamSynchronize(st));
    }
    return PV_OK;
}

extern "C" int pv_polish_summarize_regions(pv_ctx* ctx, const pv_batch_in* in, int seq_length, int seq_overlap,
                                           pv_polish_out* out) {
    PV_CHECK(ctx && in && out, PV_ERR_INVALID, "null argument");
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int G = in->n_regions;
    out->n_chunks = 0;
    out->n_rows = 0;
    if (G <= 0) return PV_OK;
    const pv_batch_shape shape = pv_check_batch(in, PV_BATCH_POLISH);
    if (shape.code) return batch_error(shape, -1);
    const int64_t n_reads = shape.n_reads, n_bases = shape.n_bases, n_cigar = shape.n_cigar, n_cols = shape.n_cols;

    pv_batch_in d;
    int rc;
    if ((rc = upload_arrays(ctx, in, shape, &d, st))) return rc;
    d.cand_start = d.ref_start; d.cand_end = d.ref_end;   // (ref, quals and the candidate bounds are not read by the polisher kernels)

    const int64_t ccap = out->chunk_capacity > 0 ? out->chunk_capacity : 0, rcap = out->flat_images ? out->row_capacity : 0;
    pv_polish_out dout = *out;
    dout.chunk_capacity = ccap;
    dout.row_capacity = rcap;
    const size_t L = (size_t)seq_length;
    if ((rc = pv_get(ctx, "pout.images", (ccap + 1) * L * 10, &dout.images))) return rc;
    if ((rc = pv_get(ctx, "pout.position", (ccap + 1) * L, &dout.position))) return rc;
    if ((rc = pv_get(ctx, "pout.index", (ccap + 1) * L, &dout.index))) return rc;
    if ((rc = pv_get(ctx, "pout.region", (size_t)ccap + 1, &dout.region))) return rc;
    if ((rc = pv_get(ctx, "pout.chunk_id", (size_t)ccap + 1, &dout.chunk_id))) return rc;
    if (out->depth)
        if ((rc = pv_get(ctx, "pout.depth", (ccap + 1) * L, &dout.depth))) return rc;
    if (out->counts)
        if ((rc = pv_get(ctx, "pout.counts", (ccap + 1) * L * 10, &dout.counts))) return rc;
    dout.flat_images = nullptr; dout.flat_position = nullptr; dout.flat_index = nullptr; dout.region_row_off = nullptr;
    if (out->flat_images) {
        PV_CHECK(out->flat_position && out->flat_index, PV_ERR_INVALID, "flat_position / flat_index missing");
        if ((rc = pv_get(ctx, "pout.flat_images", (size_t)(rcap + 1) * 10, &dout.flat_images))) return rc;
        if ((rc = pv_get(ctx, "pout.flat_position", (size_t)rcap + 1, &dout.flat_position))) return rc;
        if ((rc = pv_get(ctx, "pout.flat_index", (size_t)rcap + 1, &dout.flat_index))) return rc;
    }
    if (out->region_row_off)
        if ((rc = pv_get(ctx, "pout.region_row_off", (size_t)G + 1, &dout.region_row_off))) return rc;
    int64_t* d_counts = nullptr;
    if ((rc = pv_get(ctx, "out.counts", (size_t)4, &d_counts))) return rc;

    // workspace heuristics first; when they prove too small, what the device measured
    int64_t mp, mi;
    polish_limits(n_cols, n_bases, n_reads, &mp, &mi);
    if (rcap > n_cols && rcap - n_cols > mi) mi = rcap - n_cols;
    rc = launch_and_count(
        ctx, d_counts, st, nullptr,
        [&] { return polish_launch(ctx, &d, n_reads, n_bases, n_cigar, n_cols, mp, mi, seq_length, seq_overlap, &dout, d_counts, st); },
        [&](const int64_t* counts) {
            mp = n_reads * ((n_cols + TILE_COLS - 1) / TILE_COLS + 2);
            if (counts[3] > mi) mi = counts[3];
        });
    if (rc) return rc;
    out->n_chunks = ctx->h_counts[0];
    out->n_rows = ctx->h_counts[1];
    if (out->n_chunks > ccap || (out->flat_images && out->n_rows > rcap)) {
        pv_set_error("output capacity too small: need %lld chunks, %lld rows", (long long)out->n_chunks, (long long)out->n_rows);
        return PV_ERR_CAPACITY;
    }
    const size_t n = (size_t)out->n_chunks;
    if (n > 0 && out->images) {
        PV_HIP(hipMemcpyAsync(out->images, dout.images, n * L * 10, hipMemcpyDeviceToHost, st));
        PV_HIP(hipMemcpyAsync(out->position, dout.position, n * L * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        PV_HIP(hipMemcpyAsync(out->index, dout.index, n * L * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        PV_HIP(hipMemcpyAsync(out->region, dout.region, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        PV_HIP(hipMemcpyAsync(out->chunk_id, dout.chunk_id, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (out->depth) PV_HIP(hipMemcpyAsync(out->depth, dout.depth, n * L * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
        if (out->counts) PV_HIP(hipMemcpyAsync(out->counts, dout.counts, n * L * 10 * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
    }
    if (out->flat_images && out->n_rows > 0) {
        const size_t nr = (size_t)out->n_rows;
        PV_HIP(hipMemcpyAsync(out->flat_images, dout.flat_images, nr * 10, hipMemcpyDeviceToHost, st));
        PV_HIP(hipMemcpyAsync(out->flat_position, dout.flat_position, nr * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        PV_HIP(hipMemcpyAsync(out->flat_index, dout.flat_index, nr * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    if (out->region_row_off)
        PV_HIP(hipMemcpyAsync(out->region_row_off, dout.region_row_off, (size_t)(G + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    PV_HIP(hipStreamSynchronize(st));
    return PV_OK;
}
