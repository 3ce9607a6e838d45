// polish_filter.hip — the polisher's run filters: P2 labels + a value per edit column + draft bytes -> labels (and row
// qualities) that spell the draft over every run of adjacent edits whose lowest value is below a minimum. Two values:
//   the minimum quality (pv_polish_filter_low_qual):    the column's row quality, the top byte of column_edit's word
//   the minimum support (pv_polish_filter_low_support): the reads that spell the edit, alt_fwd + alt_rev of the evidence
//                                                       record, from the builder's counts row of the edit's own column
//
// The rules are in include/pepper_hip.h. A filter runs between the network (and the minimum-depth mask) and the stitch and
// rewrites labels only, so the stitch, quality and edit kernels behind it need no change and stay consistent with each other.
// An edit is applied whole or not at all: the unit is a run, a maximal stretch of a region's edit records (the edits' own
// column_edit on owned columns, in chunk-major = (position, index) order) whose positions are equal or consecutive. A run may
// pass through any number of chunks, so its minimum is carried across them:
//
//   k_filter_runs   one block per chunk: classify the owned columns, settle the runs that begin and end inside the chunk with
//                   a segmented min-scan (RunSum, an associative summary of a stretch of records), count their rows, and
//                   leave the chunk's summary: its first and last record, the minimum and pinned flag of its first and of its
//                   last run, whether all of it is one run
//   k_filter_carry  one block: prefix and suffix scan of the chunk summaries, runs cut where the region changes -> for every
//                   chunk the final verdict on its first and on its last run, then the counters and the status
//   k_filter_write  one block per chunk, under status PV_OK only: the same classification and scan, the verdicts of the open
//                   runs from k_filter_carry, and the rewrite. In place, rows that keep their label are not stored.
//
// k_filter_runs and k_filter_write are templated on where a record's value comes from (SUP: the counts row, loaded for edit
// columns only, after the classification); the run machinery and k_filter_carry are one. Three launches, no global atomics,
// no host synchronisation.
#include "polish_stitch_common.hpp"

using namespace pv_chunks;

namespace {

constexpr int FL_CARRY_THREADS = 1024;

// a run's verdict word: the minimum value in the low 20 bits (a quality is below 2^8, a support below 2^17), bit 20: pinned
// (an index-0 record over a draft byte no label spells). Per record, k_filter_* add bit 21: the run holds the chunk's first
// record, bit 22: it holds the chunk's last.
constexpr uint32_t RUN_VALUE = 0xfffffu, RUN_NEUTRAL = RUN_VALUE, RUN_PINNED = 1u << 20, RUN_OPEN_L = 1u << 21, RUN_OPEN_R = 1u << 22;

__device__ inline uint32_t run_merge(uint32_t x, uint32_t y) { return min(x & RUN_VALUE, y & RUN_VALUE) | ((x | y) & RUN_PINNED); }

// a stretch of edit records in order: associative under run_combine, the empty stretch is the identity
struct RunSum {
    int64_t first, last;        // positions of the first and last record
    int32_t g_first, g_last;    // their regions
    uint32_t head, tail;        // verdict words of the first and of the last run (the same run when single)
    uint32_t has, single;       // any record; all records are one run
};

__device__ inline RunSum run_empty() {
    RunSum s;
    s.first = s.last = 0; s.g_first = s.g_last = 0; s.head = s.tail = RUN_NEUTRAL; s.has = 0; s.single = 1;
    return s;
}

__device__ inline RunSum run_combine(const RunSum& x, const RunSum& y) {
    if (!x.has) return y;
    if (!y.has) return x;
    const bool joined = x.g_last == y.g_first && y.first - x.last <= 1;
    RunSum s;
    s.first = x.first; s.g_first = x.g_first; s.last = y.last; s.g_last = y.g_last; s.has = 1;
    s.head = joined && x.single ? run_merge(x.head, y.head) : x.head;
    s.tail = joined && y.single ? run_merge(x.tail, y.tail) : y.tail;
    s.single = joined && x.single && y.single;
    return s;
}

// the record of an edit column (column_edit's word e) at position p, with the value the filter judges it by
__device__ inline RunSum run_record(int64_t p, int32_t e, uint32_t value) {
    const uint32_t w = (uint32_t)e, kind = w & 0xffu, d = (w >> 8) & 0xffu;
    const uint32_t u = d >= 'a' && d <= 'z' ? d - 32 : d;
    const bool pinned = kind != PV_EDIT_INS && !(u == 'A' || u == 'C' || u == 'G' || u == 'T');
    RunSum s;
    s.first = s.last = p; s.g_first = s.g_last = 0; s.has = 1; s.single = 1;
    s.head = s.tail = value | (pinned ? RUN_PINNED : 0u);
    return s;
}

// block scan of one RunSum per thread, in thread order (REV: from the last thread down) -> the combination of the threads
// before this one (REV: behind it), exclusive; *total: all of them. In place in lds [NT], Hillis-Steele.
template <int NT, bool REV>
__device__ inline RunSum run_block_scan(RunSum mine, RunSum* lds, RunSum* total) {
    const int i = REV ? NT - 1 - (int)threadIdx.x : (int)threadIdx.x;
    lds[i] = mine;
    __syncthreads();
    for (int d = 1; d < NT; d <<= 1) {
        RunSum other = mine;
        if (i >= d) other = lds[i - d];
        __syncthreads();
        if (i >= d) {
            mine = REV ? run_combine(mine, other) : run_combine(other, mine);
            lds[i] = mine;
        }
        __syncthreads();
    }
    *total = lds[NT - 1];
    RunSum excl = run_empty();
    if (i > 0) excl = lds[i - 1];
    __syncthreads();   // lds may be reused by the caller's next scan
    return excl;
}

// what the filter kernels read and write beside the stitch's arguments and the edits' references
struct FilterArgs {
    uint8_t* lab_out;
    const uint8_t* qual_in;   // the quality plane that is copied and zeroed (null with qual_out: the support filter without one)
    uint8_t* qual_out;
    int min_value;            // min_qual or min_support
    const uint16_t* rowc;     // SUP: chunks->counts, [row][10]
    RunSum* sum;          // [n_chunks] the chunk's records, regions filled in
    int4* cnt;            // [n_chunks] rows of inner runs reverted, of inner runs pinned and low, of the first run, of the last
    uint32_t* head_fin;   // [n_chunks] verdict word of the chunk's first run, over all the chunks it passes through
    uint32_t* tail_fin;   // [n_chunks] the same of its last run
};

// the value of edit column i of this thread: its quality (in column_edit's word) or its support (in sup[])
template <bool SUP>
__device__ __forceinline__ uint32_t value_of(const int32_t* es, const uint32_t* sup, int i) {
    return SUP ? sup[i] : (uint32_t)es[i] >> 24;
}

// the chunk's columns of this thread -> es[i] (column_edit), i < n. SUP: sup[i] = the support of edit column i, from its
// counts row, which is loaded for edit columns only
template <bool SUP>
__device__ inline int classify(const StitchArgs& a, const EditRefs& r, const FilterArgs& f, const ChunkView& v, int64_t k, int j0,
                               int32_t* es, uint32_t* sup, int* bad_label, int* bad_pos) {
    const int32_t g = a.region[k];
    const int64_t o0 = r.ref_off[g], span = r.ref_off[g + 1] - o0;
    const int j1 = min(a.L, j0 + a.cpt);
    for (int j = j0; j < j1; j++) {
        const int32_t e = column_edit(a, r, v, r.ref + o0, span, j);
        es[j - j0] = e;
        *bad_label |= e == COL_BAD_LABEL;
        *bad_pos |= e == COL_BAD_POS;
        if (SUP && is_edit(e)) {
            const uint2 alt = edit_alt_counts(counts_row(f.rowc, v.base + j), e);
            sup[j - j0] = alt.x + alt.y;   // two uint16: at most 131070, compared as it is
        }
    }
    return max(0, j1 - j0);
}

// the runs of one chunk's records, as far as the chunk sees them: w[i] for edit column i of this thread = the verdict word of
// its run over the chunk's own records | RUN_OPEN_L | RUN_OPEN_R. -> the summary of the whole chunk (regions 0).
template <bool SUP>
__device__ inline RunSum chunk_runs(const StitchArgs& a, int64_t base, const int32_t* es, const uint32_t* sup, int n, RunSum* lds,
                                    uint32_t* w) {
    RunSum mine = run_empty();
    for (int i = 0; i < n; i++)
        if (is_edit(es[i])) mine = run_combine(mine, run_record(a.pos[base + i], es[i], value_of<SUP>(es, sup, i)));
    RunSum total, unused;
    RunSum run = run_block_scan<ST_THREADS, false>(mine, lds, &total);
    RunSum back = run_block_scan<ST_THREADS, true>(mine, lds, &unused);
    for (int i = 0; i < n; i++)
        if (is_edit(es[i])) {   // the run from its first record in the chunk up to this one
            run = run_combine(run, run_record(a.pos[base + i], es[i], value_of<SUP>(es, sup, i)));
            w[i] = run.tail | (run.single ? RUN_OPEN_L : 0u);
        }
    for (int i = n - 1; i >= 0; i--)
        if (is_edit(es[i])) {   // and from this one to its last
            back = run_combine(run_record(a.pos[base + i], es[i], value_of<SUP>(es, sup, i)), back);
            w[i] = run_merge(w[i], back.head) | (w[i] & RUN_OPEN_L) | (back.single ? RUN_OPEN_R : 0u);
        }
    return total;
}

template <bool SUP>
__global__ __launch_bounds__(ST_THREADS) void k_filter_runs(StitchArgs a, EditRefs r, FilterArgs f) {
    __shared__ RunSum lds[ST_THREADS];
    __shared__ int32_t lds_cnt[ST_THREADS / 64];
    const int64_t k = blockIdx.x;
    const bool ordered = chunk_in_order(a, k);
    int32_t es[ST_MAX_CPT];
    uint32_t w[ST_MAX_CPT], sup[SUP ? ST_MAX_CPT : 1];
    int n = 0, bad_label = 0, bad_pos = 0;
    const int j0 = threadIdx.x * a.cpt;
    if (ordered) n = classify<SUP>(a, r, f, chunk_view(a, k), k, j0, es, sup, &bad_label, &bad_pos);
    RunSum total = chunk_runs<SUP>(a, k * a.L + j0, es, sup, n, lds, w);
    int inner_rev = 0, inner_pin = 0, n_head = 0, n_tail = 0;
    for (int i = 0; i < n; i++)
        if (is_edit(es[i])) {
            const bool low = (int)(w[i] & RUN_VALUE) < f.min_value;
            if (w[i] & RUN_OPEN_L) n_head++;
            else if (w[i] & RUN_OPEN_R) n_tail++;
            else if (low) (w[i] & RUN_PINNED ? inner_pin : inner_rev)++;
        }
    int32_t t_rev, t_pin, t_head, t_tail, nlabel, npos;
    block_excl_scan<ST_THREADS, int32_t>(inner_rev, lds_cnt, &t_rev);
    block_excl_scan<ST_THREADS, int32_t>(inner_pin, lds_cnt, &t_pin);
    block_excl_scan<ST_THREADS, int32_t>(n_head, lds_cnt, &t_head);
    block_excl_scan<ST_THREADS, int32_t>(n_tail, lds_cnt, &t_tail);
    block_excl_scan<ST_THREADS, int32_t>(bad_label, lds_cnt, &nlabel);
    block_excl_scan<ST_THREADS, int32_t>(bad_pos, lds_cnt, &npos);
    if (threadIdx.x == 0) {
        total.g_first = total.g_last = a.region[k];
        f.sum[k] = total;
        f.cnt[k] = make_int4(t_rev, t_pin, t_head, t_tail);
        a.chunk_bad[k] = (!ordered || npos) ? BAD_ORDER : (nlabel ? BAD_LABEL : BAD_NONE);
    }
}

// one block: every chunk's first and last run joined with what stands before and behind the chunk; counters and status
__global__ __launch_bounds__(FL_CARRY_THREADS) void k_filter_carry(StitchArgs a, FilterArgs f) {
    __shared__ RunSum lds[FL_CARRY_THREADS];
    __shared__ int64_t lds_cnt[FL_CARRY_THREADS / 64];
    __shared__ int64_t s_bad[2];
    const int64_t n = a.n_chunks;
    const int64_t per = (n + FL_CARRY_THREADS - 1) / FL_CARRY_THREADS;
    const int64_t k0 = min<int64_t>(n, threadIdx.x * per), k1 = min<int64_t>(n, k0 + per);
    RunSum mine = run_empty();
    int64_t first_bad = INT64_MAX, bad_kind = BAD_NONE;
    for (int64_t k = k0; k < k1; k++) {
        mine = run_combine(mine, f.sum[k]);
        if (a.chunk_bad[k] != BAD_NONE && first_bad == INT64_MAX) { first_bad = k; bad_kind = a.chunk_bad[k]; }
    }
    RunSum unused;
    RunSum run = run_block_scan<FL_CARRY_THREADS, false>(mine, lds, &unused);
    RunSum back = run_block_scan<FL_CARRY_THREADS, true>(mine, lds, &unused);
    // what joins a chunk's last run from behind, parked in tail_fin for the pass below (same thread, same chunks)
    for (int64_t k = k1 - 1; k >= k0; k--) {
        const RunSum s = f.sum[k];
        const bool joined = s.has && back.has && back.g_first == s.g_last && back.first - s.last <= 1;
        f.tail_fin[k] = joined ? back.head : RUN_NEUTRAL;
        back = run_combine(s, back);
    }
    int64_t rev = 0, pin = 0;
    for (int64_t k = k0; k < k1; k++) {
        const RunSum s = f.sum[k];
        const uint32_t right = f.tail_fin[k];
        const bool joined = s.has && run.has && run.g_last == s.g_first && s.first - run.last <= 1;
        const uint32_t left = joined ? run.tail : RUN_NEUTRAL;
        uint32_t h = run_merge(s.head, left), t = run_merge(s.tail, right);
        if (s.single) h = t = run_merge(h, t);
        f.head_fin[k] = h;
        f.tail_fin[k] = t;
        const int4 c = f.cnt[k];
        rev += c.x;
        pin += c.y;
        if ((int)(h & RUN_VALUE) < f.min_value) (h & RUN_PINNED ? pin : rev) += c.z;
        if ((int)(t & RUN_VALUE) < f.min_value) (t & RUN_PINNED ? pin : rev) += c.w;   // (0 rows when the chunk is one run)
        run = run_combine(run, s);
    }
    int64_t n_rev, n_pin, nbad_before, nbad;
    block_excl_scan<FL_CARRY_THREADS, int64_t>(rev, lds_cnt, &n_rev);
    block_excl_scan<FL_CARRY_THREADS, int64_t>(pin, lds_cnt, &n_pin);
    // first bad chunk, as in k_stitch_scan: the segments are in chunk order, so the first thread with one holds it
    nbad_before = block_excl_scan<FL_CARRY_THREADS, int64_t>(first_bad != INT64_MAX ? 1 : 0, lds_cnt, &nbad);
    if (nbad == 0 && threadIdx.x == 0) { s_bad[0] = -1; s_bad[1] = BAD_NONE; }
    if (first_bad != INT64_MAX && nbad_before == 0) { s_bad[0] = first_bad; s_bad[1] = bad_kind; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int64_t kind = s_bad[1];
        const int64_t status = kind == BAD_ORDER ? PV_ERR_INVALID : kind == BAD_LABEL ? PV_ERR_STATE : PV_OK;
        a.counts[0] = status == PV_OK ? n_rev : 0;
        a.counts[1] = status;
        a.counts[2] = s_bad[0];
        a.counts[3] = status == PV_OK ? n_pin : 0;
    }
}

template <bool SUP>
__global__ __launch_bounds__(ST_THREADS) void k_filter_write(StitchArgs a, EditRefs r, FilterArgs f) {
    __shared__ RunSum lds[ST_THREADS];
    if (a.counts[1] != PV_OK) return;
    const int64_t k = blockIdx.x;
    int32_t es[ST_MAX_CPT];
    uint32_t w[ST_MAX_CPT], sup[SUP ? ST_MAX_CPT : 1];
    int bad_label = 0, bad_pos = 0;   // (status OK: no COL_BAD code can come back)
    const int j0 = threadIdx.x * a.cpt;
    const int n = classify<SUP>(a, r, f, chunk_view(a, k), k, j0, es, sup, &bad_label, &bad_pos);
    const int64_t base = k * a.L + j0;
    chunk_runs<SUP>(a, base, es, sup, n, lds, w);
    const uint32_t head = f.head_fin[k], tail = f.tail_fin[k];
    const bool lab_copy = f.lab_out != a.lab, qual_copy = f.qual_out != f.qual_in;
    for (int i = 0; i < n; i++) {
        const int64_t t = base + i;
        bool revert = false;
        if (is_edit(es[i])) {
            const uint32_t v = w[i] & RUN_OPEN_L ? head : w[i] & RUN_OPEN_R ? tail : w[i];
            revert = (int)(v & RUN_VALUE) < f.min_value && !(v & RUN_PINNED);
        }
        if (revert) {
            const uint32_t e = (uint32_t)es[i], d = (e >> 8) & 0xffu, u = d >= 'a' && d <= 'z' ? d - 32 : d;
            // (an index-0 record of a run that is not pinned stands over A, C, G or T)
            f.lab_out[t] = (e & 0xffu) == PV_EDIT_INS ? 0 : u == 'A' ? 1 : u == 'C' ? 2 : u == 'G' ? 3 : 4;
            if (!SUP || f.qual_out) f.qual_out[t] = 0;
        } else {
            if (lab_copy) f.lab_out[t] = a.lab[t];
            if (qual_copy) f.qual_out[t] = f.qual_in[t];
        }
    }
}

// what both forms of a filter refuse before they touch the device: the threshold, the quality planes, the chunk geometry
int filter_check(bool sup, int min_value, const uint8_t* row_qual, const uint8_t* row_qual_out, int seq_length, int seq_overlap) {
    if (sup) {
        PV_CHECK(min_value >= 0 && min_value <= 65535, PV_ERR_INVALID, "filter: min_support %d is outside 0..65535", min_value);
        PV_CHECK(!row_qual == !row_qual_out, PV_ERR_INVALID,
                 "filter: row_qual and row_qual_out are given or null together (one of them is null)");
    } else {
        PV_CHECK(min_value >= 0 && min_value <= 94, PV_ERR_INVALID, "filter: min_qual %d is outside 0..94", min_value);
        PV_CHECK(row_qual && row_qual_out, PV_ERR_INVALID, "filter: the row qualities are missing (row_qual or row_qual_out is null)");
    }
    PV_CHECK(seq_length >= 1 && seq_length <= ST_THREADS * ST_MAX_CPT && seq_overlap >= 0 && seq_overlap < seq_length,
             PV_ERR_INVALID, "filter: need 1 <= seq_length <= %d and 0 <= seq_overlap < seq_length (got %d, %d)",
             ST_THREADS * ST_MAX_CPT, seq_length, seq_overlap);
    PV_CHECK(2 * seq_overlap <= seq_length, PV_ERR_INVALID, "filter: a column may overlap one neighbour chunk only (overlap %d)",
             seq_overlap);
    return PV_OK;
}

// both device forms. sup: the support filter, whose values come from chunks->counts (else the quality filter's, from row_qual)
int filter_launch(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const uint8_t* labels, const uint8_t* row_qual,
                  const int64_t* region_start, const int64_t* ref_off, const uint8_t* ref, int32_t n_regions, int seq_length,
                  int seq_overlap, int min_value, uint8_t* labels_out, uint8_t* row_qual_out, int64_t* d_counts, void* stream,
                  bool sup) {
    PV_CHECK(ctx && chunks && d_counts, PV_ERR_INVALID, "null argument");
    PV_CHECK(n_chunks >= 0 && n_regions >= 0, PV_ERR_INVALID, "negative sizes");
    int rc;
    if ((rc = filter_check(sup, min_value, row_qual, row_qual_out, seq_length, seq_overlap))) return rc;
    if (sup) {
        PV_CHECK(n_chunks == 0 || (chunks->depth && chunks->counts), PV_ERR_INVALID,
                 "filter: the chunks carry no depth plane or no counts plane (pv_polish_out.depth, .counts)");
        PV_CHECK(((uintptr_t)chunks->counts & 3) == 0, PV_ERR_INVALID, "counts is not aligned to 4 bytes");
    }
    PV_CHECK(n_chunks <= chunks->chunk_capacity, PV_ERR_INVALID, "n_chunks %lld exceeds the chunk capacity %lld",
             (long long)n_chunks, (long long)chunks->chunk_capacity);
    PV_CHECK(n_chunks < (1ll << 31), PV_ERR_LIMIT, "too many chunks for one launch");
    PV_CHECK(n_chunks == 0 || ref, PV_ERR_INVALID, "filter: the batch carries no draft bytes (ref is null)");
    PV_CHECK(n_chunks == 0 || (chunks->position && chunks->index && chunks->region && chunks->chunk_id && labels && labels_out &&
                               region_start && ref_off && n_regions > 0),
             PV_ERR_INVALID, "chunk arrays, labels, region starts or draft offsets missing");
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = pv_pick_stream(ctx, stream);
    StitchArgs a = chunk_args(chunks, labels, region_start, n_chunks, n_regions, seq_length, seq_overlap, d_counts);
    // the support filter classifies without the quality byte: it judges by the counts row and only copies and zeroes qualities
    EditRefs r = {ref_off, ref, sup ? nullptr : row_qual};
    FilterArgs f = {labels_out, row_qual, row_qual_out, min_value, sup ? chunks->counts : nullptr, nullptr, nullptr, nullptr, nullptr};
    const size_t nk = (size_t)(n_chunks > 0 ? n_chunks : 1);
    if ((rc = pv_get(ctx, "filter.bad", nk, &a.chunk_bad))) return rc;
    if ((rc = pv_get(ctx, "filter.sum", nk, &f.sum))) return rc;
    if ((rc = pv_get(ctx, "filter.cnt", nk, &f.cnt))) return rc;
    if ((rc = pv_get(ctx, "filter.head", nk, &f.head_fin))) return rc;
    if ((rc = pv_get(ctx, "filter.tail", nk, &f.tail_fin))) return rc;
    const unsigned nb = (unsigned)n_chunks;
    if (sup) {
        pv_prof_scope ps_all(ctx, "polish_filter_support", st);
        if (n_chunks > 0) { pv_prof_scope ps(ctx, "k_filter_runs_support", st); k_filter_runs<true><<<nb, ST_THREADS, 0, st>>>(a, r, f); }
        k_filter_carry<<<1, FL_CARRY_THREADS, 0, st>>>(a, f);
        if (n_chunks > 0) { pv_prof_scope ps(ctx, "k_filter_write_support", st); k_filter_write<true><<<nb, ST_THREADS, 0, st>>>(a, r, f); }
    } else {
        pv_prof_scope ps_all(ctx, "polish_filter", st);
        if (n_chunks > 0) { pv_prof_scope ps(ctx, "k_filter_runs", st); k_filter_runs<false><<<nb, ST_THREADS, 0, st>>>(a, r, f); }
        k_filter_carry<<<1, FL_CARRY_THREADS, 0, st>>>(a, f);
        if (n_chunks > 0) { pv_prof_scope ps(ctx, "k_filter_write", st); k_filter_write<false><<<nb, ST_THREADS, 0, st>>>(a, r, f); }
    }
    PV_HIP(hipGetLastError());
    return PV_OK;
}

// both host forms
int filter_host(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const uint8_t* labels, const uint8_t* row_qual,
                const int64_t* region_start, const int64_t* ref_off, const uint8_t* ref, int32_t n_regions, int seq_length,
                int seq_overlap, int min_value, uint8_t* labels_out, uint8_t* row_qual_out, int64_t* counts, bool sup) {
    PV_CHECK(ctx && chunks && counts, PV_ERR_INVALID, "null argument");
    PV_CHECK(n_chunks >= 0 && n_regions >= 0 && seq_length >= 1, PV_ERR_INVALID, "negative sizes");
    int rc;   // everything the call itself refuses is refused here, before a byte is copied to the device
    if ((rc = filter_check(sup, min_value, row_qual, row_qual_out, seq_length, seq_overlap))) return rc;
    PV_CHECK(!sup || n_chunks == 0 || (chunks->depth && chunks->counts), PV_ERR_INVALID,
             "filter: the chunks carry no depth plane or no counts plane (pv_polish_out.depth, .counts)");
    PV_CHECK(n_chunks == 0 || (ref_off && n_regions > 0), PV_ERR_INVALID, "draft offsets missing");
    PV_CHECK(n_chunks == 0 || ref, PV_ERR_INVALID, "filter: the batch carries no draft bytes (ref is null)");
    PV_CHECK(n_chunks == 0 || (labels && labels_out), PV_ERR_INVALID, "labels missing");
    PV_CHECK(!ref_off || ref_off[n_regions] >= 0, PV_ERR_INVALID, "negative draft length");
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t nc = (size_t)n_chunks, L = (size_t)seq_length;
    pv_polish_out d;
    uint8_t *d_lab = nullptr, *d_rq = nullptr, *d_ref = nullptr, *d_lab_out = nullptr, *d_rq_out = nullptr;
    int64_t *d_rs = nullptr, *d_ro = nullptr, *d_counts = nullptr;
    if (row_qual && (rc = stage(ctx, "fl.row_qual", row_qual, nc * L, &d_rq, st))) return rc;
    if ((rc = stage_chunks(ctx, "fl", chunks, nc, L, sup && nc > 0, sup && nc > 0, &d, st))) return rc;   // (no chunks: no planes)
    if ((rc = stage(ctx, "fl.labels", labels, nc * L, &d_lab, st))) return rc;
    if ((rc = stage_draft(ctx, "fl", region_start, ref_off, ref, n_regions, &d_rs, &d_ro, &d_ref, st))) return rc;
    // in place on the host is in place on the device
    d_lab_out = d_lab;
    if (labels_out != labels && (rc = pv_get(ctx, "fl.labels_out", nc * L > 0 ? nc * L : 1, &d_lab_out))) return rc;
    d_rq_out = d_rq;
    if (row_qual && row_qual_out != row_qual && (rc = pv_get(ctx, "fl.row_qual_out", nc * L > 0 ? nc * L : 1, &d_rq_out))) return rc;
    if ((rc = pv_get(ctx, "fl.counts", (size_t)4, &d_counts))) return rc;
    rc = filter_launch(ctx, &d, n_chunks, d_lab, d_rq, d_rs, d_ro, d_ref, n_regions, seq_length, seq_overlap, min_value, d_lab_out,
                       d_rq_out, d_counts, st, sup);
    if (rc) return rc;
    PV_HIP(hipMemcpyAsync(counts, d_counts, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    PV_HIP(hipStreamSynchronize(st));
    const int64_t status = counts[1];
    PV_CHECK(status != PV_ERR_STATE, PV_ERR_STATE, "filter: chunk %lld holds a label outside 0..4 (a poisoned network result)",
             (long long)counts[2]);
    PV_CHECK(status != PV_ERR_INVALID, PV_ERR_INVALID,
             "filter: chunk %lld breaks the layout (regions ascending, chunk ids 0,1,2,... inside a region, positions inside the "
             "region's draft bytes)", (long long)counts[2]);
    PV_CHECK(status == PV_OK, (int)status, "filter: device status %lld", (long long)status);
    if (nc * L > 0) {
        PV_HIP(hipMemcpyAsync(labels_out, d_lab_out, nc * L, hipMemcpyDeviceToHost, st));
        if (row_qual_out) PV_HIP(hipMemcpyAsync(row_qual_out, d_rq_out, nc * L, hipMemcpyDeviceToHost, st));
        PV_HIP(hipStreamSynchronize(st));
    }
    return PV_OK;
}

}  // namespace

extern "C" int pv_polish_filter_low_qual_dev(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const uint8_t* labels,
                                             const uint8_t* row_qual, const int64_t* region_start, const int64_t* ref_off,
                                             const uint8_t* ref, int32_t n_regions, int seq_length, int seq_overlap, int min_qual,
                                             uint8_t* labels_out, uint8_t* row_qual_out, int64_t* d_counts, void* stream) {
    return filter_launch(ctx, chunks, n_chunks, labels, row_qual, region_start, ref_off, ref, n_regions, seq_length, seq_overlap,
                         min_qual, labels_out, row_qual_out, d_counts, stream, false);
}

extern "C" int pv_polish_filter_low_qual(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const uint8_t* labels,
                                         const uint8_t* row_qual, const int64_t* region_start, const int64_t* ref_off,
                                         const uint8_t* ref, int32_t n_regions, int seq_length, int seq_overlap, int min_qual,
                                         uint8_t* labels_out, uint8_t* row_qual_out, int64_t* counts) {
    return filter_host(ctx, chunks, n_chunks, labels, row_qual, region_start, ref_off, ref, n_regions, seq_length, seq_overlap,
                       min_qual, labels_out, row_qual_out, counts, false);
}

extern "C" int pv_polish_filter_low_support_dev(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const uint8_t* labels,
                                                const uint8_t* row_qual, const int64_t* region_start, const int64_t* ref_off,
                                                const uint8_t* ref, int32_t n_regions, int seq_length, int seq_overlap,
                                                int min_support, uint8_t* labels_out, uint8_t* row_qual_out, int64_t* d_counts,
                                                void* stream) {
    return filter_launch(ctx, chunks, n_chunks, labels, row_qual, region_start, ref_off, ref, n_regions, seq_length, seq_overlap,
                         min_support, labels_out, row_qual_out, d_counts, stream, true);
}

extern "C" int pv_polish_filter_low_support(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const uint8_t* labels,
                                            const uint8_t* row_qual, const int64_t* region_start, const int64_t* ref_off,
                                            const uint8_t* ref, int32_t n_regions, int seq_length, int seq_overlap, int min_support,
                                            uint8_t* labels_out, uint8_t* row_qual_out, int64_t* counts) {
    return filter_host(ctx, chunks, n_chunks, labels, row_qual, region_start, ref_off, ref, n_regions, seq_length, seq_overlap,
                       min_support, labels_out, row_qual_out, counts, true);
}
