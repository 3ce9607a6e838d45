// polish_stitch_common.hpp — what the passes over the polisher's labelled chunks share (polish_stitch.hip, polish_edits.hip, ...):
// the kernel arguments, the chunk layout contract, the decimal string order of chunk ids, the block scan, the one-block scan
// of the per-chunk counts into offsets and status, the edit rule of one column (polish_edits.hip, polish_filter.hip), and the
// host form's staging copy.
#pragma once
#include "pv_common.hpp"

namespace pv_chunks {

constexpr int ST_THREADS = 256;
constexpr int ST_MAX_CPT = 16;        // columns per thread: seq_length <= 4096
constexpr int ST_SCAN_THREADS = 1024;
constexpr int64_t ST_BUFFER = 200;    // 2 * ImageSizeOptions.MIN_IMAGE_OVERLAP (Stitch.py:42)

enum { BAD_NONE = 0, BAD_LABEL = 1, BAD_ORDER = 2 };

struct StitchArgs {
    const int64_t* pos;
    const int32_t* idx;
    const int32_t* region;
    const int32_t* cid;
    const uint8_t* lab;
    const int64_t* rstart;
    int64_t n_chunks;
    int n_regions;
    int L;
    int step;      // seq_length - seq_overlap
    int cpt;       // columns per thread
    int32_t* chunk_cnt;
    int32_t* chunk_bad;
    int64_t* chunk_off;
    int64_t* region_off;
    uint8_t* seq;
    int64_t cap;
    int64_t* counts;
};

// str(a) > str(b) for a, b >= 0 (Python string order of the decimal forms)
__device__ inline bool dec_str_gt(int32_t a, int32_t b) {
    int na = 1, nb = 1;
    for (int32_t v = a; v >= 10; v /= 10) na++;
    for (int32_t v = b; v >= 10; v /= 10) nb++;
    if (na == nb) return a > b;
    if (na < nb) {
        int32_t pb = b;
        for (int i = na; i < nb; i++) pb /= 10;  // the first na digits of b
        return a > pb;                            // equal: a is a proper prefix of b, so it sorts first
    }
    int32_t pa = a;
    for (int i = nb; i < na; i++) pa /= 10;
    return pa >= b;                               // equal: b is a proper prefix of a
}

// the chunk layout contract: regions ascending, a region's chunks contiguous with ids 0, 1, 2, ...
__device__ inline bool chunk_in_order(const StitchArgs& a, int64_t k) {
    const int32_t g = a.region[k], c = a.cid[k];
    if (g < 0 || g >= a.n_regions || c < 0) return false;
    if (k == 0) return c == 0;
    const int32_t pg = a.region[k - 1];
    return pg == g ? c == a.cid[k - 1] + 1 : (pg < g && c == 0);
}

struct ChunkView {
    int64_t base;      // k * L
    int64_t rs;        // region start
    bool prev, next;   // the neighbouring chunk of the same region exists
    int32_t c, cprev, cnext;
};

__device__ inline ChunkView chunk_view(const StitchArgs& a, int64_t k) {
    ChunkView v;
    v.base = k * a.L;
    const int32_t g = a.region[k];
    v.rs = a.rstart[g];
    v.c = a.cid[k];
    v.prev = k > 0 && a.region[k - 1] == g;
    v.next = k + 1 < a.n_chunks && a.region[k + 1] == g;
    v.cprev = v.prev ? a.cid[k - 1] : 0;
    v.cnext = v.next ? a.cid[k + 1] : 0;
    return v;
}

// what the edit kernels read beside the stitch's arguments
struct EditRefs {
    const int64_t* ref_off;
    const uint8_t* ref;
    const uint8_t* row_qual;   // may be null: qual 255
};

enum { COL_NONE = 0, COL_BAD_LABEL = -1, COL_BAD_POS = -2 };

// > 0: an edit, packed as the record's last word (kind | draft << 8 | base << 16 | qual << 24); else a COL_ code.
// span: the bytes of this region's draft. The draft byte is loaded for owned index-0 columns only, inside [0, span).
__device__ inline int32_t column_edit(const StitchArgs& a, const EditRefs& r, const ChunkView& v, const uint8_t* draft, int64_t span,
                                      int j) {
    const int64_t t = v.base + j;
    const int64_t p = a.pos[t];
    const int32_t x = a.idx[t];
    if (p < 0 || x < 0) return COL_NONE;
    if (v.rs > 0 && p <= v.rs + ST_BUFFER) return COL_NONE;
    const int ov = a.L - a.step;
    if (v.prev && j < ov) {   // also column j + step of the previous chunk
        const int64_t u = t - a.L + a.step;
        if (a.pos[u] == p && a.idx[u] == x && !dec_str_gt(v.c, v.cprev)) return COL_NONE;
    }
    if (v.next && j >= a.step) {   // also column j - step of the next chunk
        const int64_t u = t + a.L - a.step;
        if (a.pos[u] == p && a.idx[u] == x && !dec_str_gt(v.c, v.cnext)) return COL_NONE;
    }
    const int64_t rel = p - v.rs;
    if (rel < 0 || rel >= span) return COL_BAD_POS;
    const uint32_t lb = a.lab[t];
    if (lb > 4) return COL_BAD_LABEL;
    uint32_t kind, d = 0, base = lb ? (uint32_t)"ACGT"[lb - 1] : 0;
    if (x > 0) {
        if (lb == 0) return COL_NONE;
        kind = PV_EDIT_INS;
    } else {
        d = draft[rel];
        const uint32_t u = d >= 'a' && d <= 'z' ? d - 32 : d;
        if (lb == 0) kind = PV_EDIT_DEL;
        else if (base != u) kind = PV_EDIT_SUB;
        else return COL_NONE;
    }
    const uint32_t q = r.row_qual ? r.row_qual[t] : 255u;
    return (int32_t)(kind | d << 8 | base << 16 | q << 24);   // q <= 255 and kind >= 1: bit 31 may be set, so test != codes
}

__device__ inline bool is_edit(int32_t e) { return e != COL_NONE && e != COL_BAD_LABEL && e != COL_BAD_POS; }

// one row of the builder's counts plane (pv_polish_out.counts, [row][10] uint16) held as five dwords, and count f (0..9) of
// it. 20 bytes a row: dword aligned when the plane is. row_count takes the row by value and picks the dword with masks, so
// that no address of a member is ever selected: a `?:` or an `if` over the members becomes an indexed load of the struct,
// which then lives in scratch or, promoted, in 20 bytes of LDS per lane. Like this the row stays in registers (the kernels'
// LDS is their scans' alone).
struct CountsRow { uint32_t w0, w1, w2, w3, w4; };
__device__ __forceinline__ CountsRow counts_row(const uint16_t* counts, int64_t t) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(counts + t * 10);
    return CountsRow{src[0], src[1], src[2], src[3], src[4]};
}
__device__ __forceinline__ uint32_t row_count(CountsRow w, uint32_t f) {
    const uint32_t h = f >> 1;
    const uint32_t x = (w.w0 & (0u - (h == 0))) | (w.w1 & (0u - (h == 1))) | (w.w2 & (0u - (h == 2))) | (w.w3 & (0u - (h == 3))) |
                       (w.w4 & (0u - (h == 4)));
    return (f & 1 ? x >> 16 : x) & 0xFFFFu;
}
// 0..3 for A C G T (upper case), else 4
__device__ __forceinline__ uint32_t acgt_index(uint32_t c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u; }

// the reads that spell the edit `e` (column_edit's word) in its own counts row: x = alt_fwd, y = alt_rev of the edit's
// pv_polish_evidence record (the rule is in pepper_hip.h). x + y is the edit's SUPPORT (pv_polish_filter_low_support).
__device__ __forceinline__ uint2 edit_alt_counts(const CountsRow& w, int32_t e) {
    const uint32_t kind = (uint32_t)e & 0xFF, base = ((uint32_t)e >> 16) & 0xFF;
    const uint32_t k = acgt_index(base), f_rev = kind == PV_EDIT_DEL ? 8u : k, f_fwd = kind == PV_EDIT_DEL ? 9u : 4u + k;
    return make_uint2(row_count(w, f_fwd), row_count(w, f_rev));
}

// exclusive block scan; *total gets the block's sum. NT threads, NT/64 waves.
template <int NT, typename T>
__device__ inline T block_excl_scan(T v, T* lds, T* total) {
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
#pragma unroll
    for (int i = 0; i < NT / 64; i++) {
        off += i < w ? lds[i] : 0;
        sum += lds[i];
    }
    __syncthreads();   // lds may be reused by the caller's next scan
    *total = sum;
    return off + x - v;
}

// one block: chunk offsets, region offsets, total, status and the first bad chunk
static __global__ __launch_bounds__(ST_SCAN_THREADS) void k_stitch_scan(StitchArgs a) {
    __shared__ int64_t lds[ST_SCAN_THREADS / 64];
    const int64_t n = a.n_chunks;
    const int64_t per = (n + ST_SCAN_THREADS - 1) / ST_SCAN_THREADS;
    const int64_t k0 = min<int64_t>(n, threadIdx.x * per), k1 = min<int64_t>(n, k0 + per);
    int64_t s = 0, first_bad = INT64_MAX, bad_kind = BAD_NONE, n_unordered = 0;
    for (int64_t k = k0; k < k1; k++) {
        s += a.chunk_cnt[k];
        n_unordered += a.chunk_bad[k] == BAD_ORDER;
        if (a.chunk_bad[k] != BAD_NONE && first_bad == INT64_MAX) { first_bad = k; bad_kind = a.chunk_bad[k]; }
    }
    int64_t total, any_unordered;
    int64_t off = block_excl_scan<ST_SCAN_THREADS, int64_t>(s, lds, &total);
    block_excl_scan<ST_SCAN_THREADS, int64_t>(n_unordered, lds, &any_unordered);
    // first bad chunk: the segments are in chunk order, so the first thread with one holds it
    int64_t nbad_before, nbad;
    nbad_before = block_excl_scan<ST_SCAN_THREADS, int64_t>(first_bad != INT64_MAX ? 1 : 0, lds, &nbad);
    __shared__ int64_t s_bad[2];
    if (nbad == 0 && threadIdx.x == 0) { s_bad[0] = -1; s_bad[1] = BAD_NONE; }
    if (first_bad != INT64_MAX && nbad_before == 0) { s_bad[0] = first_bad; s_bad[1] = bad_kind; }
    __syncthreads();
    const int64_t bad_chunk = s_bad[0], kind = s_bad[1];
    const int64_t status = kind == BAD_ORDER ? PV_ERR_INVALID : kind == BAD_LABEL ? PV_ERR_STATE
                   : total > a.cap ? PV_ERR_CAPACITY : PV_OK;
    for (int64_t k = k0; k < k1; k++) {
        a.chunk_off[k] = off;
        if (!any_unordered) {   // (region ids are only known to be in range then)
            // region g's bases start at its first chunk; regions without chunks take the next one's offset
            const int32_t g = a.region[k], pg = k > 0 ? a.region[k - 1] : -1;
            for (int32_t r = pg + 1; r <= g; r++) a.region_off[r] = off;
        }
        off += a.chunk_cnt[k];
    }
    if (threadIdx.x == 0) {
        if (!any_unordered) {
            const int32_t g_last = n > 0 ? a.region[n - 1] : -1;
            for (int32_t r = g_last + 1; r <= a.n_regions; r++) a.region_off[r] = total;
        }
        a.counts[0] = total;
        a.counts[1] = status;
        a.counts[2] = bad_chunk;
        a.counts[3] = 0;
    }
}

// what every pass's launcher fills of the kernel arguments: the chunk arrays, the labels (null where the pass reads none), the
// region starts, the sizes and the counters. The per-chunk arrays and a pass's own outputs are the launcher's to add.
inline StitchArgs chunk_args(const pv_polish_out* chunks, const uint8_t* labels, const int64_t* region_start, int64_t n_chunks,
                             int32_t n_regions, int seq_length, int seq_overlap, int64_t* d_counts) {
    StitchArgs a;
    memset(&a, 0, sizeof(a));
    a.pos = chunks->position; a.idx = chunks->index; a.region = chunks->region; a.cid = chunks->chunk_id;
    a.lab = labels; a.rstart = region_start;
    a.n_chunks = n_chunks; a.n_regions = n_regions;
    a.L = seq_length; a.step = seq_length - seq_overlap; a.cpt = (seq_length + ST_THREADS - 1) / ST_THREADS;
    a.counts = d_counts;
    return a;
}

// the block's smallest `bad` (INT64_MAX: no thread has one), in thread 0 only: the wave minimum, then the waves' minima by one
// thread. NT threads; lds holds NT/64 entries of its own.
template <int NT>
__device__ inline int64_t block_first_bad(int64_t bad, int64_t* lds) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int64_t y = __shfl_xor(bad, d, 64);
        bad = y < bad ? y : bad;
    }
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = bad;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int i = 1; i < NT / 64; i++) bad = lds[i] < bad ? lds[i] : bad;
    return bad;
}

constexpr int ST_FINISH_THREADS = 1024;

// one block, for a pass that counts two things per chunk (the mask, the vote): the sums of a.chunk_cnt and chunk_cnt2, the
// status and the first bad chunk -> d_counts. A bad chunk zeroes both sums.
static __global__ __launch_bounds__(ST_FINISH_THREADS) void k_chunk_finish(StitchArgs a, const int32_t* chunk_cnt2) {
    __shared__ int64_t lds[ST_FINISH_THREADS / 64];
    __shared__ int64_t s_bad[ST_FINISH_THREADS / 64];
    int64_t n = 0, n2 = 0, bad = INT64_MAX;
    for (int64_t k = threadIdx.x; k < a.n_chunks; k += ST_FINISH_THREADS) {
        n += a.chunk_cnt[k];
        n2 += chunk_cnt2[k];
        if (a.chunk_bad[k] != BAD_NONE && k < bad) bad = k;
    }
    int64_t total, total2, nbad;
    block_excl_scan<ST_FINISH_THREADS, int64_t>(n, lds, &total);
    block_excl_scan<ST_FINISH_THREADS, int64_t>(n2, lds, &total2);
    block_excl_scan<ST_FINISH_THREADS, int64_t>(bad != INT64_MAX ? 1 : 0, lds, &nbad);
    bad = block_first_bad<ST_FINISH_THREADS>(bad, s_bad);
    if (threadIdx.x == 0) {
        a.counts[0] = nbad ? 0 : total;
        a.counts[1] = nbad ? PV_ERR_INVALID : PV_OK;
        a.counts[2] = nbad ? bad : -1;
        a.counts[3] = nbad ? 0 : total2;
    }
}

// the host forms' upload of one input array into a named workspace slot
template <typename T>
static int stage(pv_ctx* ctx, const char* name, const T* src, size_t n, T** dst, hipStream_t st) {
    int rc = pv_get(ctx, name, n > 0 ? n : 1, dst);
    if (rc) return rc;
    if (n > 0) PV_HIP(hipMemcpyAsync(*dst, src, n * sizeof(T), hipMemcpyHostToDevice, st));
    return PV_OK;
}

// the host forms' upload of the chunk arrays of nc chunks of L rows into the slots <prefix>.position, .index, .region and
// .chunk_id and, where the pass reads them, .depth and .rowcounts -> *d, the device's pv_polish_out
static int stage_chunks(pv_ctx* ctx, const char* prefix, const pv_polish_out* chunks, size_t nc, size_t L, bool want_depth,
                        bool want_counts, pv_polish_out* d, hipStream_t st) {
    const std::string p(prefix);
    memset(d, 0, sizeof(*d));
    d->chunk_capacity = (int64_t)nc;
    int rc;
    if ((rc = stage(ctx, (p + ".position").c_str(), (const int64_t*)chunks->position, nc * L, &d->position, st))) return rc;
    if ((rc = stage(ctx, (p + ".index").c_str(), (const int32_t*)chunks->index, nc * L, &d->index, st))) return rc;
    if ((rc = stage(ctx, (p + ".region").c_str(), (const int32_t*)chunks->region, nc, &d->region, st))) return rc;
    if ((rc = stage(ctx, (p + ".chunk_id").c_str(), (const int32_t*)chunks->chunk_id, nc, &d->chunk_id, st))) return rc;
    if (want_depth && (rc = stage(ctx, (p + ".depth").c_str(), (const uint16_t*)chunks->depth, nc * L, &d->depth, st))) return rc;
    if (want_counts && (rc = stage(ctx, (p + ".rowcounts").c_str(), (const uint16_t*)chunks->counts, nc * L * 10, &d->counts, st)))
        return rc;
    return PV_OK;
}

// the host forms' upload of the draft triple into the slots <prefix>.region_start, .ref_off and .ref. ref_off or ref may be
// null (the device form refuses that where it has chunks): nothing is copied for it.
static int stage_draft(pv_ctx* ctx, const char* prefix, const int64_t* region_start, const int64_t* ref_off, const uint8_t* ref,
                       int32_t n_regions, int64_t** d_rs, int64_t** d_ro, uint8_t** d_ref, hipStream_t st) {
    const std::string p(prefix);
    const size_t n_ref = ref_off && ref ? (size_t)ref_off[n_regions] : 0;
    int rc;
    if ((rc = stage(ctx, (p + ".region_start").c_str(), region_start, (size_t)n_regions, d_rs, st))) return rc;
    if ((rc = stage(ctx, (p + ".ref_off").c_str(), ref_off, ref_off ? (size_t)n_regions + 1 : 0, d_ro, st))) return rc;
    return stage(ctx, (p + ".ref").c_str(), ref, n_ref, d_ref, st);
}

}  // namespace pv_chunks
