// summary_builder.hip — the pileup summary-image builder on gfx950 (MI355X).
//
// Replaces RegionalSummaryGenerator::generate_summary + populate_summary_matrix
// (reference: pepper_variant/modules/cpp/region_summary.cpp:337-566, 568-916) for a whole BATCH of
// regions per call. It is an HBM-bound integer pipeline; nothing here is GEMM-shaped.
//
// Data layout in HBM (column = one reference position; global column id = ref_off[g] + i):
//   cnt[n_cols][CNT_STRIDE] int16, COLUMN-MAJOR since round 3 (the 21 counters of a column are 48 contiguous bytes: only the
//   columns something reads - sites and the windows around them, ~20 % - are written at all, by one thread each in three 16-byte
//   stores, and a window's 33 columns are one 1.6 KB run; they were [NCNT][n_cols] planes, every column of every plane written)
//   (cnt_t: a count is bounded by the reads of its region, which k_init holds to <= 32767 - the
//   reference's caller keeps at most MAX_READS_IN_REGION = 5000, pepper_variant/modules/python/Options.py:98); counter index inside a column:
//     0 coverage  1 snp_count  2 insert_count  3 delete_count  4 rare-event count
//     5 + 8*strand + {0 REF, 1 A, 2 C, 3 G, 4 T, 5 I, 6 D, 7 *}   (the 16 accumulated planes of the
//     reference's 26; planes 0-3,5-7,16-18 are constants or overlays and are never stored)
//   the clamp of planes 11..24 (region_summary.cpp:648-653) is applied when windows are gathered, so
//   the raw counters stay available as exact SNP allele counts.
//
// Pipeline (all on one stream, no host round trip in the middle):
//   k_cigar_scan     wave per read: prefix sums over CIGAR ops -> per-op (column, read index)
//   k_tile_fill      lane per (read, 512-column tile): op range of the read that can touch the tile
//   k_pileup_tiles   workgroup per tile: counters in LDS, aligned bases dealt to lanes in padded groups of 4
//   (site flags: frequency thresholds per column, per-tile site counts - in the flush of k_pileup_tiles)
//   k_scan_*         single-block exclusive scans (tiny arrays)
//   k_site_rank      site columns -> site list (rank = tile offset + rank inside the 1024-column block), per-site event bucket sizes
//   k_collect        wave per site, lane per overlapping read: the read's ops at that column by binary search; allele events
//   k_site_alleles   wave per site: dedupe + order alleles like std::set<std::string>, filters
//   k_write_windows  wave per site: gather 33x26, clamp, overlays, int8 cast, metadata, keys
//
// Allele keys never leave their source: an allele is (type, length, pointer into bases/ref), compared
// bytewise exactly as std::string operator< would compare "<type digit><bytes>".
#include "summary_launch.hpp"
#include "summary_scan.hpp"

namespace pvsum {
namespace {

// Does the insert of `len` bases whose anchor base is bases[ins_start] count (region_summary.cpp:431-490 /
// region_summary_hp.cpp:469-553)? The quality sum runs over the anchor base and the inserted bases (26-plane form) or over the
// inserted bases only (haplotag form). k_pileup_tiles counts it into the planes of its anchor column, k_collect repeats the
// test at site columns instead of reading a per-op flag (scattered one-byte stores: ~30 MB of HBM writes per 16 regions).
__device__ __forceinline__ bool insert_counts(const SumArgs& a, int64_t ins_start, int32_t len, bool hp) {
    const int64_t L = (int64_t)len + 1;
    int64_t qs_all = 0;
    for (int64_t i = 0; i < L; i++) qs_all += a.in.quals[ins_start + i];
    const int q0 = a.in.quals[ins_start];
    if (hp) return 2 + (int64_t)len <= PV_MAX_ALLELE_KEY && (double)(qs_all - q0) >= a.p.min_indel_baseq * (double)len;
    return 1 + L <= PV_MAX_ALLELE_KEY && (double)qs_all >= a.p.min_indel_baseq * (double)L;
}

// events per site -> offsets, total -> diag[D_NEVENTS]; site / event workspace limits. Grid: scan_chunks(max_sites).
__global__ __launch_bounds__(1024) void k_scan_events(SumArgs a) {
    __shared__ int64_t s_w[32];
    const int64_t c0 = (int64_t)blockIdx.x * SCAN_PASS, i0 = c0 + (int64_t)threadIdx.x * SCAN_V;
    const bool spec = blockIdx.x < SCAN_SPEC_CHUNKS;
    int32_t v[SCAN_V];
    scan_load(a.site_nev, i0, a.max_sites, v);
    const int64_t n_raw = scan_len_issue(a.diag + D_NSITES);
    int64_t part = spec ? scan_carry_part_spec(a.site_nev, c0) : 0;
    const int64_t n_sites = scan_len_uniform(n_raw);
    const int64_t n = n_sites > a.max_sites ? a.max_sites : n_sites;
    if (c0 >= n && blockIdx.x > 0) return;
    if (!spec) part = scan_carry_part(a.site_nev, c0, a.max_sites);
    scan_mask(i0, n, v);
    const int64_t total = scan_pass(v, a.site_evoff, i0, n, 0, part, s_w);
    if (threadIdx.x == 0 && n <= c0 + SCAN_PASS) {
        a.diag[D_NEVENTS] = total;
        if (n_sites > a.max_sites || total > a.max_events) set_status(a.diag, PV_ERR_LIMIT);
    }
}

// windows and key bytes per site -> offsets, totals -> diag[D_NOUT], diag[D_STRBYTES]; result counters of the call.
// Grid: scan_chunks(max_sites).
__global__ __launch_bounds__(1024) void k_scan_outputs(SumArgs a) {
    __shared__ int64_t s_w[2][32];
    const int64_t c0 = (int64_t)blockIdx.x * SCAN_PASS, i0 = c0 + (int64_t)threadIdx.x * SCAN_V;
    const bool spec = blockIdx.x < SCAN_SPEC_CHUNKS;
    int32_t ve[SCAN_V];
    int64_t vs[SCAN_V];
    scan_load(a.site_nemit, i0, a.max_sites, ve);
    scan_load(a.site_strbytes, i0, a.max_sites, vs);
    const int64_t n_raw = scan_len_issue(a.diag + D_NSITES);
    int64_t pe = 0, ps = 0;
    if (spec) {
        pe = scan_carry_part_spec(a.site_nemit, c0);
        ps = scan_carry_part_spec(a.site_strbytes, c0);
    }
    const int64_t n_sites = scan_len_uniform(n_raw);
    const int64_t n = n_sites > a.max_sites ? a.max_sites : n_sites;
    if (c0 >= n && blockIdx.x > 0) return;
    if (!spec) {
        pe = scan_carry_part(a.site_nemit, c0, a.max_sites);
        ps = scan_carry_part(a.site_strbytes, c0, a.max_sites);
    }
    const int64_t status = a.diag[D_STATUS];  // (k_write_windows, the only kernel behind this one, sets no status)
    scan_mask(i0, n, ve);
    scan_mask(i0, n, vs);
    const int64_t n_out = scan_pass(ve, a.site_outoff, i0, n, 0, pe, s_w[0]);
    const int64_t n_str = scan_pass(vs, a.site_stroff, i0, n, 0, ps, s_w[1]);
    if (threadIdx.x == 0 && n <= c0 + SCAN_PASS) {
        a.diag[D_NOUT] = n_out;
        a.diag[D_STRBYTES] = n_str;
        a.d_counts[0] = n_out;
        a.d_counts[1] = n_str;
        a.d_counts[2] = status;
        a.d_counts[3] = n_sites;
    }
}

__global__ __launch_bounds__(1024) void k_site_rank(SumArgs a) {
    __shared__ int32_t s_w[16], s_p[16];
    const int64_t col = (int64_t)blockIdx.x * 1024 + threadIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int f = col < a.n_cols ? a.flags[col] : 0;
    // sites before this block = the per-tile counts (k_pileup_tiles) of the tiles before it, added up here (at most 3 k values,
    // three coalesced loads per thread) instead of by a scan kernel of its own in front of this one
    const int64_t tiles_before = (int64_t)blockIdx.x * (1024 / TILE_COLS);
    int part = 0;
    for (int64_t i = threadIdx.x; i < tiles_before; i += 1024) part += a.blk_cnt[i];
    const int pinc = wave_incl_scan32(part, lane);
    const int site = f & 1;
    const unsigned long long m = __ballot(site);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_w[wv] = __popcll(m);
    if (lane == 63) s_p[wv] = pinc;
    __syncthreads();
    int woff = 0, own = 0, base = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        woff += k < wv ? s_w[k] : 0;
        own += s_w[k];
        base += s_p[k];
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) a.diag[D_NSITES] = (int64_t)base + own;   // the last block knows the total
    const int32_t rank = base + woff + before;
    if (site && rank < a.max_sites) {
        int g = a.tile_g0[col / TILE_COLS];   // region of the tile's first column (k_init), then forwards: two dependent loads, not five
        while (g + 1 <= a.in.n_regions && a.in.ref_off[g + 1] <= col) g++;
        a.site_col[rank] = (int32_t)col;
        a.site_region[rank] = g;
        // events a site will receive: every insert / delete observation, and either the rare SNP observations (the
        // common ones are read off the symbol planes) or, in the haplotag form, every SNP observation
        const cnt_t* cc = a.cnt + (int64_t)col * (a.hp ? CNT_STRIDE_HP : CNT_STRIDE);   // this column's counters
        const int n_base = cc[a.hp ? C_SNP : C_RARE];
        const int nev = cc[C_INS] + cc[C_DEL] + n_base;
        a.site_nev[rank] = nev;
        a.site_fill[rank] = 0;
        SiteHdr h;
        h.col = (int32_t)col; h.col_base = (int32_t)a.in.ref_off[g]; h.g = g;
        h.ref_start = a.in.ref_start[g];
        h.R = (int32_t)(a.in.ref_end[g] - h.ref_start + 1);
        const int64_t t = col / TILE_COLS;
        h.p0 = a.tile_off[t]; h.np = a.tile_cnt[t];
        h.cov = cc[C_COV];
        h.flags = (int32_t)a.in.ref[col] | (n_base != 0 ? 256 : 0) | (f << 16);
        h.nev = nev; h.pad = 0;
        a.site_hdr[rank] = h;
        // the few sites whose events exceed the small allele table are listed for the large-table launch of k_site_alleles
        if (nev + 4 > UM_SMALL) a.big_sites[atomicAdd((unsigned long long*)&a.diag[D_NBIG], 1ull)] = rank;
    }
}

// ---- K5 -------------------------------------------------------------------------------------------
// Site-indexed kernels walk the site list XCD by XCD: workgroup b runs on XCD b & 7 (round-robin dispatch), so giving
// each XCD one contiguous eighth of the sites, in order, keeps the sites of a tile - which read the same pair records,
// the same op ranges (the upper probes of their binary searches are the same words) and neighbouring counter columns -
// in ONE 4 MB L2 at about the same time instead of fetching them into up to eight. Grids are multiples of 8.
__device__ __forceinline__ int64_t xcd_chunk(int64_t n_sites) { return (n_sites + 7) >> 3; }
__device__ __forceinline__ int64_t xcd_site(int64_t j, int64_t n_sites) { return (int64_t)(blockIdx.x & 7) * xcd_chunk(n_sites) + j; }

// (nev, evoff: the site's bucket size and offset, read once per site by the caller)
__device__ __forceinline__ void push_event(const SumArgs& a, int32_t s, int32_t nev, int64_t evoff, int64_t src, int32_t len,
                                           int type, bool rev, int kind, int flags) {
    const int32_t slot = atomicAdd(&a.site_fill[s], 1);
    if (slot >= nev) { set_status(a.diag, PV_ERR_INVALID); return; }  // cannot happen: exact bucket sizes
    Event e;
    e.src = src; e.len = len; e.type = (uint8_t)type; e.rev = rev ? 1 : 0; e.kind = (uint8_t)kind; e.flags = (uint8_t)flags;
    a.ev[evoff + slot] = e;
}

// One WAVE per SITE, one lane per (read, tile) pair of the site's tile: the allele observations a read contributes at that
// column. Sites are ~1 column in 200, so walking the CIGAR stream a second time (a workgroup per read, five loads per op,
// 20 M ops per launch) spent nearly all its loads on ops that touch no site; here a lane finds the read's ops at the site
// column with one binary search over the pair's op range (start columns are sorted), 8 k sites x ~70 reads x 7 steps.
//   ops that START right behind the column and are inserts / deletes anchor on it (counted by k_pileup_tiles: insert_counts());
//   the aligned op that contains the column gives the read's base there (rare observations only, or - haplotag form - every
//   mismatch).
constexpr int KC_WAVES = 2;  // waves per site: the benchmark's tiles hold ~70 pairs, which one wave would walk as two trips in a row
__global__ __launch_bounds__(64 * KC_WAVES) void k_collect(SumArgs a) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (a.diag[D_STATUS] != 0) return;
    int64_t n_sites = a.diag[D_NSITES];
    if (n_sites > a.max_sites) n_sites = a.max_sites;
    for (int64_t sj = blockIdx.x >> 3; sj < xcd_chunk(n_sites); sj += gridDim.x >> 3) {
        const int64_t s = xcd_site(sj, n_sites);
        if (s >= n_sites) break;
        const SiteHdr h = a.site_hdr[s];
        const int64_t evoff = a.site_evoff[s];
        const int64_t col = h.col;
        const int64_t col_base = h.col_base;
        const int32_t col_rel = (int32_t)(col - col_base);
        const bool need_base = (h.flags & 256) != 0;
        const int refb = h.flags & 0xFF;
        const int sub_k = (int)(col & (TILE_COLS - 1)) / SUB_COLS;
        const int32_t p0 = h.p0, np = h.np;
        for (int32_t pb = 64 * wv; pb < np; pb += 64 * KC_WAVES) {
            if (pb + lane >= np) continue;
            const PairRec pr = a.pairs[p0 + pb + lane];
            if (pr.col_base != (int32_t)col_base) continue;   // a tile can hold the end of one region and the start of the next
            const bool rev = (pr.rev & 1) != 0;
            int obs = 1;  // flags of an allele observation
            if (a.hp) obs |= ((pr.rev >> 1) & 3) << 2;         // count sets of the read (k_tile_fill)
            // first op of the pair's range that starts behind the column; the pair's sub-tile index narrows the range to the ops
            // between the 64-column boundaries around the site (every op before the first starts before the boundary at or before
            // the column, no op from the second on starts at or before the column)
            int32_t lo = pr.op_lo, hi = pr.op_hi;
            if (pr.sub(SUB_N + 1)) {
                lo += pr.sub(sub_k);
                const int s1 = pr.sub(sub_k + 1);
                if (s1 < 255 && pr.op_lo + s1 < hi) hi = pr.op_lo + s1;
            }
            while (lo < hi) { const int32_t mid = (lo + hi) >> 1; if (a.op_ref[mid] <= col_rel) lo = mid + 1; else hi = mid; }
            const int32_t f = lo;
            for (int32_t o = f; o < pr.op_hi; o++) {            // inserts / deletes anchored on the column
                if (a.op_ref[o] != col_rel + 1) break;
                const uint32_t w = a.in.cigar[o];
                const int op = w & 0xF;
                const int32_t len = (int32_t)(w >> 4);
                if (op == PV_CIGAR_IN) {   // the conditions under which k_pileup_tiles counted it (INS plane, insert_count)
                    const int32_t rdv = a.op_rd[o];
                    const int64_t ins_start = pr.base0 + rdv - 1;
                    if (rdv >= 1 && ins_start + (int64_t)len + 1 <= pr.seq_end && insert_counts(a, ins_start, len, a.hp != 0))
                        push_event(a, (int32_t)s, h.nev, evoff, ins_start, len + 1, 2, rev, 1, obs);
                } else if (op == PV_CIGAR_DEL) {
                    int64_t L = (int64_t)len + 1;
                    if ((int64_t)col_rel + L > pr.ref_len) L = pr.ref_len - col_rel;
                    if (1 + L <= PV_MAX_ALLELE_KEY) push_event(a, (int32_t)s, h.nev, evoff, col, (int32_t)L, 3, rev, 2, obs);
                }
            }
            if (!need_base) continue;
            for (int32_t o = f - 1; o >= pr.op_lo; o--) {       // the op that holds the column, skipping ops that consume no reference
                const uint32_t w = a.in.cigar[o];
                const int op = w & 0xF;
                const bool aligned = op == PV_CIGAR_MATCH || op == PV_CIGAR_EQUAL || op == PV_CIGAR_DIFF;
                if (!aligned) {
                    if (op == PV_CIGAR_DEL || op == PV_CIGAR_REF_SKIP || op == PV_CIGAR_PAD) break;   // the column lies in a gap of this read
                    continue;
                }
                const int32_t rr = a.op_ref[o];
                const int64_t i = (int64_t)col_rel - rr;
                if (rr == OP_INACTIVE || i < 0 || i >= (int64_t)(w >> 4)) break;
                const int64_t bi = pr.base0 + a.op_rd[o] + i;
                if (bi >= pr.seq_end) break;  // already reported by k_pileup
                const int base = a.in.bases[bi];
                if (!((double)a.in.quals[bi] >= a.p.min_snp_baseq)) break;
                if (a.hp) {  // every mismatch (raw bytes, region_summary_hp.cpp:406) is an allele observation
                    if (refb != base) push_event(a, (int32_t)s, h.nev, evoff, bi, 1, 1, rev, 1, obs);
                    break;
                }
                const bool refvalid = is_acgt(up(refb));
                const bool rare = (refb != base) && !(refvalid && is_acgt(base));
                const bool corr = refvalid && base != up(base) && is_acgt(up(base));
                if (rare || corr) push_event(a, (int32_t)s, h.nev, evoff, bi, 1, 1, rev, 1, (rare ? 1 : 0) | (corr ? 2 : 0));
                break;
            }
        }
    }
}

// ---- K6 -------------------------------------------------------------------------------------------
struct Key {
    int64_t src;
    int32_t len;
    uint8_t type, kind, imm;
};
__device__ __forceinline__ int key_byte(const SumArgs& a, const Key& k, int i) {
    return k.kind == 0 ? k.imm : (k.kind == 1 ? a.in.bases[k.src + i] : a.in.ref[k.src + i]);
}
// the first (up to) 8 bytes of a key, big-endian and zero-padded, so that integer order is byte order: fetched ONCE per
// allele; nearly every comparison (SNP keys are one byte, most indels a few) is then decided in registers / LDS instead of
// with dependent byte loads from the bases / reference
__device__ __forceinline__ uint64_t key_prefix(const SumArgs& a, const Key& k) {
    uint64_t p = 0;
    const int n = k.len < 8 ? k.len : 8;
    for (int i = 0; i < n; i++) p |= (uint64_t)(uint8_t)key_byte(a, k, i) << (56 - 8 * i);
    return p;
}
// std::string compare of "<type digit><bytes>" given the prefixes: equal prefixes mean the first min(len, 8) bytes agree
// (where a zero byte meets padding the shorter key is a prefix of the longer, which the length rule orders the same way)
__device__ __forceinline__ int key_cmp(const SumArgs& a, const Key& x, uint64_t px, const Key& y, uint64_t py) {
    if (x.type != y.type) return x.type < y.type ? -1 : 1;
    if (px != py) return px < py ? -1 : 1;
    const int m = x.len < y.len ? x.len : y.len;
    for (int i = 8; i < m; i++) {
        const int bx = key_byte(a, x, i), by = key_byte(a, y, i);
        if (bx != by) return bx < by ? -1 : 1;
    }
    if (x.len != y.len) return x.len < y.len ? -1 : 1;
    return 0;
}

// HP: the haplotag form keeps four per-strand counts per allele (forward / reverse x haplotype set 1 / 2,
// region_summary_hp.cpp:415-447) next to the total, and no allele count comes from the planes.
// UM = alleles the LDS table of a wave holds. The table is what limits the waves per CU (1024 entries are 34 KB: four waves
// per CU, one per SIMD, and a site is a chain of dependent loads), while a site can never hold more distinct alleles than it
// has events + 4: sites with few events (all but the deepest) run in the instantiation with a UM_SMALL-entry table, BIG = the
// others.
template <bool HP, int UM, bool BIG>
__global__ __launch_bounds__(64) void k_site_alleles(SumArgs a) {
    __shared__ int64_t u_src[UM];
    __shared__ uint64_t u_pre[UM];  // key_prefix of the allele
    __shared__ int32_t u_len[UM];
    __shared__ int32_t u_fwd[UM];   // HP: total observations
    __shared__ int32_t u_rev[UM];   // HP: unused (0), so that u_fwd + u_rev is the total in both forms
    __shared__ int32_t u_hc[HP ? 4 : 1][HP ? UM : 1];  // HP: forward set 1, forward set 2, reverse set 1, reverse set 2
    __shared__ uint8_t u_type[UM];
    __shared__ uint8_t u_kind[UM];
    __shared__ uint8_t u_imm[UM];
    __shared__ uint8_t u_ok[UM];
    __shared__ int16_t u_order[UM];
    __shared__ int32_t s_nU;
    const int lane = threadIdx.x;
    if (a.diag[D_STATUS] != 0) return;
    int64_t n_sites = a.diag[D_NSITES];
    if (n_sites > a.max_sites) n_sites = a.max_sites;
    const int64_t n_big = BIG ? a.diag[D_NBIG] : 0;
    for (int64_t sj = BIG ? blockIdx.x : blockIdx.x >> 3; sj < (BIG ? n_big : xcd_chunk(n_sites)); sj += BIG ? gridDim.x : gridDim.x >> 3) {
        const int64_t s = BIG ? a.big_sites[sj] : xcd_site(sj, n_sites);
        if (s >= n_sites) { if (BIG) continue; else break; }
        const SiteHdr h = a.site_hdr[s];
        const int64_t eoff = a.site_evoff[s];          // (requested together with the header)
        if ((h.nev + 4 > UM_SMALL) != BIG) continue;   // the other instantiation's site
        const int64_t col = h.col;
        const int f = (h.flags >> 16) & 0xFF;
        const int cov = h.cov;
        const int depth = cov < PV_MAX_COLOR ? cov : PV_MAX_COLOR;  // :682
        const int refraw = h.flags & 0xFF;
        const bool refvalid = is_acgt(up(refraw));
        __syncthreads();
        // slots 0..3: SNP alleles whose counts are the (negated, un-clamped) A/C/G/T planes
        if (!HP && lane < 4) {
            const int b = "ACGT"[lane];
            u_src[lane] = 0; u_len[lane] = 1; u_type[lane] = 1; u_kind[lane] = 0; u_imm[lane] = (uint8_t)b;
            u_pre[lane] = (uint64_t)(uint8_t)b << 56;
            const bool ok = refvalid && b != refraw;
            u_ok[lane] = ok;
            u_fwd[lane] = ok ? -a.cnt[(int64_t)col * CNT_STRIDE + C_PLANE + 1 + lane] : 0;
            u_rev[lane] = ok ? -a.cnt[(int64_t)col * CNT_STRIDE + C_PLANE + 8 + 1 + lane] : 0;
        }
        if (lane == 0) s_nU = HP ? 0 : 4;
        __syncthreads();
        const int nev = h.nev;
        for (int eb = 0; eb < nev; eb += 64) {
            const bool have = eb + lane < nev;
            Event e;
            e.src = 0; e.len = 0; e.type = 0; e.rev = 0; e.kind = 1; e.flags = 0;
            if (have) e = a.ev[eoff + eb + lane];
            if (!HP && have && (e.flags & 2)) {  // lower-case acgt was counted in plane toupper(): take it back out
                const int ub = up(a.in.bases[e.src]);
                const int sl = ub == 'A' ? 0 : ub == 'C' ? 1 : ub == 'G' ? 2 : 3;
                if (u_ok[sl]) atomicAdd(e.rev ? &u_rev[sl] : &u_fwd[sl], -1);
            }
            bool pending = have && (e.flags & 1);
            Key ke; ke.src = e.src; ke.len = e.len; ke.type = e.type; ke.kind = e.kind; ke.imm = 0;
            const uint64_t pe = pending ? key_prefix(a, ke) : 0;
            int checked = HP ? 0 : 4;  // slots 0..3 can never equal an event key (see k_pileup: those are not events)
            [[maybe_unused]] const int hs = (e.flags >> 2) & 3, hst = e.rev ? 2 : 0;
            while (true) {
                const int nU = s_nU;
                if (pending) {
                    for (int k = checked; k < nU; k++) {
                        Key ku; ku.src = u_src[k]; ku.len = u_len[k]; ku.type = u_type[k]; ku.kind = u_kind[k]; ku.imm = u_imm[k];
                        if (ku.type == ke.type && ku.len == ke.len && u_pre[k] == pe && key_cmp(a, ku, pe, ke, pe) == 0) {
                            if constexpr (HP) {
                                atomicAdd(&u_fwd[k], 1);
                                if (hs & 1) atomicAdd(&u_hc[hst + 0][k], 1);
                                if (hs & 2) atomicAdd(&u_hc[hst + 1][k], 1);
                            } else
                            atomicAdd(e.rev ? &u_rev[k] : &u_fwd[k], 1);
                            pending = false;
                            break;
                        }
                    }
                }
                checked = nU;
                const unsigned long long m = __ballot(pending);
                if (m == 0) break;
                const int leader = __ffsll((long long)m) - 1;
                if (lane == leader) {
                    if (nU < UM) {
                        u_src[nU] = ke.src; u_len[nU] = ke.len; u_type[nU] = ke.type; u_kind[nU] = ke.kind; u_imm[nU] = 0;
                        u_pre[nU] = pe;
                        if constexpr (HP) {
                            u_ok[nU] = 1; u_fwd[nU] = 1; u_rev[nU] = 0;
                            u_hc[0][nU] = (!e.rev && (hs & 1)) ? 1 : 0; u_hc[1][nU] = (!e.rev && (hs & 2)) ? 1 : 0;
                            u_hc[2][nU] = (e.rev && (hs & 1)) ? 1 : 0;  u_hc[3][nU] = (e.rev && (hs & 2)) ? 1 : 0;
                        } else {
                        u_ok[nU] = 1; u_fwd[nU] = e.rev ? 0 : 1; u_rev[nU] = e.rev ? 1 : 0;
                        }
                        s_nU = nU + 1;
                    } else {
                        set_status(a.diag, PV_ERR_LIMIT);
                    }
                    pending = false;
                }
                __syncthreads();
            }
            __syncthreads();
        }
        __syncthreads();
        const int nU = s_nU;
        // order like std::set<std::string> (:670): rank among the observed alleles
        int nV = 0;
        for (int kb = 0; kb < nU; kb += 64) {
            const int k = kb + lane;
            const bool live = k < nU && u_ok[k] && (u_fwd[k] + u_rev[k]) > 0;
            if (live) {
                Key kk; kk.src = u_src[k]; kk.len = u_len[k]; kk.type = u_type[k]; kk.kind = u_kind[k]; kk.imm = u_imm[k];
                const uint64_t pk = u_pre[k];
                int rank = 0;
                for (int j = 0; j < nU; j++) {
                    if (j == k || !u_ok[j] || (u_fwd[j] + u_rev[j]) <= 0) continue;
                    Key kj; kj.src = u_src[j]; kj.len = u_len[j]; kj.type = u_type[j]; kj.kind = u_kind[j]; kj.imm = u_imm[j];
                    if (key_cmp(a, kj, u_pre[j], kk, pk) < 0) rank++;
                }
                u_order[rank] = (int16_t)k;
            }
            nV += __popcll(__ballot(live));
        }
        __syncthreads();
        // filters (:682-712) in set order; survivors become allele records
        const int64_t recbase = eoff + 4 * s;
        int nemit = 0;
        int64_t sbytes = 0;
        for (int rb = 0; rb < nV; rb += 64) {
            const int r = rb + lane;
            bool keep = false;
            int k = 0;
            if (r < nV) {
                k = u_order[r];
                const int total = u_fwd[k] + u_rev[k];
                const int t = u_type[k];
                const double dd = (double)depth > 1.0 ? (double)depth : 1.0;
                const double freq = (double)total / dd;
                keep = true;
                if ((double)total < a.p.candidate_support_threshold) keep = false;
                if (t != 1 && freq < a.p.indel_candidate_freq_threshold) keep = false;
                if (t == 1 && freq < a.p.snp_candidate_freq_threshold) keep = false;
                if (t != 1 && a.p.skip_indels) keep = false;
                if ((t == 1 && !(f & 2)) || (t == 2 && !(f & 4)) || (t == 3 && !(f & 8))) keep = false;
            }
            const unsigned long long m = __ballot(keep);
            if (keep) {
                const int e = nemit + __popcll(m & ((1ull << lane) - 1ull));
                AlleleRec rc;
                rc.src = u_src[k]; rc.len = u_len[k]; rc.total = u_fwd[k] + u_rev[k]; rc.fwd = u_fwd[k]; rc.rev = u_rev[k];
                if constexpr (HP) {  // the four overlay values, already clamped (region_summary_hp.cpp:971-974)
                    auto c8 = [](int v) { return (uint32_t)(v < PV_MAX_COLOR ? v : PV_MAX_COLOR); };
                    rc.fwd = (int32_t)(c8(u_hc[0][k]) | (c8(u_hc[1][k]) << 8) | (c8(u_hc[2][k]) << 16) | (c8(u_hc[3][k]) << 24));
                    rc.rev = 0;
                }
                rc.type = u_type[k]; rc.kind = u_kind[k]; rc.imm = u_imm[k]; rc.pad = 0; rc.pad2 = 0;
                a.rec[recbase + e] = rc;
            }
            nemit += __popcll(m);
            int64_t b = keep ? 1 + u_len[k] : 0;
            for (int d = 32; d >= 1; d >>= 1) b += __shfl_xor(b, d, 64);
            sbytes += b;
        }
        if (lane == 0) {
            a.site_nemit[s] = nemit;
            a.site_strbytes[s] = sbytes;
        }
    }
}

// ---- K8 -------------------------------------------------------------------------------------------
// a window is a chain of gathers per lane: WW_THREADS lanes share one site's windows, so that a lane walks 4 elements of a
// window instead of 14 and four times as many chains are in flight per CU
constexpr int WW_THREADS = 256;
// What the two forms of a window differ in besides the candidate's overlay: geometry, the counter column behind a window
// plane, and which planes are clamped.
template <bool HP> struct WinForm;
template <> struct WinForm<false> {   // region_summary.cpp:831-904: 33 rows x 26 planes
    static constexpr int ROWS = PV_WINDOW_ROWS, FEATURES = PV_FEATURES, STRIDE = CNT_STRIDE;
    // feature -> counter plane: REF count 4 / 15, symbol planes 8..14 / 19..25; the rest is written per candidate
    static __device__ __forceinline__ int plane(int pl) {
        return pl == 4 ? C_PLANE : (pl >= 8 && pl <= 14) ? C_PLANE + 1 + (pl - 8)
             : pl == 15 ? C_PLANE + 8 : pl >= 19 ? C_PLANE + 8 + 1 + (pl - 19) : -1;
    }
    static __device__ __forceinline__ bool clamped(int pl) { return pl >= 11 && pl <= 24; }  // :648-653
};
template <> struct WinForm<true> {    // region_summary_hp.cpp:943-1003: 21 rows x 48 planes, every plane clamped (:762-767)
    static constexpr int ROWS = PV_HP_WINDOW_ROWS, FEATURES = PV_HP_FEATURES, STRIDE = CNT_STRIDE_HP;
    static __device__ __forceinline__ int plane(int pl) {
        const int grp = (pl - 4) / 11, w = (pl - 4) - 11 * grp;  // 0 REF count, 1-3 overlays, 4-10 symbols
        return pl < 4 ? -1 : (w == 0 ? HC_PLANE + 8 * grp : (w >= 4 ? HC_PLANE + 8 * grp + (w - 3) : -1));
    }
    static __device__ __forceinline__ bool clamped(int) { return true; }
};

// The candidate's own values on the middle row. 26-plane form (:848-904): allele code or length, its two strand counts, sign
// flips of the planes the allele was counted in, and - deletions - the same on the rows the deletion covers. Haplotag form
// (:970-974, :983-987, :996-1000): allele code or length and the four per-set strand counts; no deletion tail, no sign flips.
template <bool HP>
__global__ __launch_bounds__(WW_THREADS) void k_write_windows(SumArgs a) {
    using F = WinForm<HP>;
    constexpr int BYTES = F::ROWS * F::FEATURES, MID = (F::ROWS - 1) / 2;
    __shared__ int32_t s_win[BYTES];
    const int lane = threadIdx.x;
    if (a.diag[D_STATUS] != 0) return;
    int64_t n_sites = a.diag[D_NSITES];
    if (n_sites > a.max_sites) n_sites = a.max_sites;
    for (int64_t sj = blockIdx.x >> 3; sj < xcd_chunk(n_sites); sj += gridDim.x >> 3) {
        const int64_t s = xcd_site(sj, n_sites);
        if (s >= n_sites) break;
        // (everything a site's windows start from is requested at once, also for the two sites in three that emit nothing:
        // one round trip instead of two for those that do)
        const int nemit = a.site_nemit[s];
        const SiteHdr h = a.site_hdr[s];
        const int64_t evoff_s = a.site_evoff[s], stroff_s = a.site_stroff[s], outoff_s = a.site_outoff[s];
        if (nemit == 0) continue;
        const int64_t col = h.col;
        const int g = h.g;
        const int64_t col_base = h.col_base;
        const int64_t R = h.R;
        const int64_t ci = col - col_base;
        const int cov = h.cov;
        const int depth = cov < PV_MAX_COLOR ? cov : PV_MAX_COLOR;
        [[maybe_unused]] const bool refvalid = is_acgt(up(h.flags & 0xFF));
        const int64_t recbase = evoff_s + 4 * s;
        int64_t so = stroff_s;
        for (int e = 0; e < nemit; e++) {
            const AlleleRec rc = a.rec[recbase + e];
            const int64_t k = outoff_s + e;
            const int64_t send = so + 1 + rc.len;
            if (k < a.out.capacity && send <= a.out.str_capacity) {
                const int t = rc.type;  // 1 SNP, 2 INS, 3 DEL
                const int clen = rc.len < PV_MAX_COLOR ? rc.len : PV_MAX_COLOR;
                [[maybe_unused]] int cfwd = 0, crev = 0, alt = 0, ff = -1, fr = -1, end_index = 0;   // 26-plane form
                [[maybe_unused]] int v1 = 0;                                                         // haplotag form
                [[maybe_unused]] const uint32_t hc = (uint32_t)rc.fwd;  // forward set 1, forward set 2, reverse set 1, reverse set 2
                if constexpr (HP) {
                    v1 = t == 1 ? refcode(a.in.bases[rc.src]) : clen;
                } else {
                    cfwd = rc.fwd < PV_MAX_COLOR ? rc.fwd : PV_MAX_COLOR;
                    crev = rc.rev < PV_MAX_COLOR ? rc.rev : PV_MAX_COLOR;
                    if (t == 1) {
                        alt = rc.kind == 0 ? rc.imm : a.in.bases[rc.src];
                        if (refvalid) { ff = 7 + sym_of(alt); fr = 18 + sym_of(alt); }
                    } else if (t == 2) {
                        if (refvalid) { ff = 12; fr = 23; }
                    } else {
                        if (refvalid) { ff = 13; fr = 24; }
                    }
                    end_index = MID + rc.len - 1;  // :885
                    if (end_index > F::ROWS - 2) end_index = F::ROWS - 2;
                }
                // gather with the ROW running fastest across lanes: a column's counters are contiguous, so the lanes of a wave
                // read runs of consecutive columns; the finished window goes through LDS and leaves in its own (row, feature)
                // order, coalesced
                constexpr int WW_TRIPS = (BYTES + WW_THREADS - 1) / WW_THREADS;
                int raw[WW_TRIPS];
#pragma unroll
                for (int u = 0; u < WW_TRIPS; u++) {   // every load of the window is requested before the first is used
                    const int tt = lane + u * WW_THREADS;
                    const int pl = tt / F::ROWS, row = tt - pl * F::ROWS;
                    const int64_t i = ci - MID + row;
                    const bool in = tt < BYTES && i >= 0 && i < R;  // row R of the reference's matrix exists and is all zero (:835)
                    const int64_t c2 = col_base + (in ? i : 0);
                    const int plane = F::plane(pl);
                    int v = 0;
                    if (in && plane >= 0) v = a.cnt[c2 * F::STRIDE + plane];
                    if (in && pl == 0) v = a.in.ref[c2];
                    raw[u] = v;
                }
#pragma unroll
                for (int u = 0; u < WW_TRIPS; u++) {
                    const int tt = lane + u * WW_THREADS;
                    if (tt >= BYTES) continue;
                    const int pl = tt / F::ROWS, row = tt - pl * F::ROWS;
                    const int64_t i = ci - MID + row;
                    int v = raw[u];
                    if (i >= 0 && i < R) {
                        if (pl == 0) v = refcode(v);
                        if (F::clamped(pl)) v = v > PV_MAX_COLOR ? PV_MAX_COLOR : (v < -PV_MAX_COLOR ? -PV_MAX_COLOR : v);
                    }
                    if constexpr (HP) {
                        if (row == MID) {
                            if (pl == t) v = v1;
                            if (pl == 4 + t) v = (int)(hc & 0xFF);
                            if (pl == 26 + t) v = (int)((hc >> 8) & 0xFF);
                            if (pl == 15 + t) v = (int)((hc >> 16) & 0xFF);
                            if (pl == 37 + t) v = (int)((hc >> 24) & 0xFF);
                        }
                    } else {
                        if (row == MID) {  // :848-894
                            if (t == 1) {
                                if (pl == 1) v = refcode(alt);
                                if (pl == 5) v = cfwd;
                                if (pl == 16) v = crev;
                            } else if (t == 2) {
                                if (pl == 2) v = clen;
                                if (pl == 6) v = cfwd;
                                if (pl == 17) v = crev;
                            } else {
                                if (pl == 3) v = clen;
                                if (pl == 7) v = cfwd;
                                if (pl == 18) v = crev;
                            }
                            if (pl == ff || pl == fr) v = -v;
                        } else if (t == 3 && row > MID && row <= end_index) {  // :895-904
                            if (pl == 3) v = clen;
                            if (pl == 7) v = cfwd;
                            if (pl == 18) v = crev;
                            if (refvalid && (pl == 14 || pl == 25)) v = -v;
                        }
                    }
                    s_win[row * F::FEATURES + pl] = v;
                }
                __syncthreads();
                for (int el = lane; el < BYTES; el += WW_THREADS) {
                    const int v = s_win[el];
                    a.out.images[k * BYTES + el] = (int8_t)(uint8_t)(v & 0xFF);  // DataStore.py:68 wrap
                    if (a.out.images_i32) a.out.images_i32[k * BYTES + el] = v;
                }
                __syncthreads();
                if (lane == 0) {
                    a.out.region[k] = g;
                    a.out.position[k] = h.ref_start + ci;
                    a.out.depth[k] = (uint8_t)depth;
                    a.out.cand_freq[k] = (uint8_t)(rc.total < PV_MAX_COLOR ? rc.total : PV_MAX_COLOR);
                    a.out.cand_off[k] = so;
                    a.out.cand_off[k + 1] = send;
                    a.out.cand_str[so] = (char)('0' + rc.type);
                }
                for (int i = lane; i < rc.len; i += WW_THREADS) {   // (kind 0, an immediate byte: 26-plane form only)
                    const int b = (!HP && rc.kind == 0) ? rc.imm : (rc.kind == 1 ? a.in.bases[rc.src + i] : a.in.ref[rc.src + i]);
                    a.out.cand_str[so + 1 + i] = (char)b;
                }
            }
            so = send;
        }
    }
}

}  // namespace

// Workspace + launch sequence. Everything asynchronous on `st`.
int summarize_launch(pv_ctx* ctx, const pv_batch_in* in, const pv_params* params, int64_t n_reads, int64_t n_bases,
                     int64_t n_cigar, int64_t n_cols, int64_t max_sites, int64_t max_events, int64_t max_pairs,
                     const pv_batch_out* out, int64_t* d_counts, hipStream_t st, bool hp, const int32_t* read_hp) {
    if (hp)
        PV_CHECK(params->candidate_window_size == PV_HP_WINDOW_ROWS - 1 && params->feature_size == PV_HP_FEATURES,
                 PV_ERR_INVALID, "haplotag builder: candidate_window_size must be 20 and feature_size 48 (got %d, %d)",
                 params->candidate_window_size, params->feature_size);
    else
    PV_CHECK(params->candidate_window_size == 32 && params->feature_size == PV_FEATURES, PV_ERR_INVALID,
             "candidate_window_size must be 32 and feature_size 26 (got %d, %d)", params->candidate_window_size,
             params->feature_size);
    SumArgs a;
    memset(&a, 0, sizeof(a));
    a.in = *in;
    a.p = *params;
    a.n_reads = n_reads; a.n_bases = n_bases; a.n_cigar = n_cigar; a.n_cols = n_cols;
    a.max_sites = max_sites; a.max_events = max_events; a.max_pairs = max_pairs;
    a.out = *out;
    a.d_counts = d_counts;
    a.hp = hp ? 1 : 0;
    a.read_hp = read_hp;
    const int64_t n_blk = (n_cols + 1023) / 1024;
    {
        const double t = params->min_snp_baseq;
        a.qmin_snp = t <= 0.0 ? 0 : (t > 255.0 ? 256 : (int32_t)ceil(t));
    }
    int rc;
    if ((rc = front_claim(ctx, a))) return rc;
    if ((rc = pv_get(ctx, "sum.cnt", (size_t)(hp ? CNT_STRIDE_HP : CNT_STRIDE) * n_cols, &a.cnt))) return rc;
    if ((rc = pv_get(ctx, "sum.flags", n_cols, &a.flags))) return rc;
    if ((rc = pv_get(ctx, "sum.blk_cnt", (size_t)a.n_tiles + 2, &a.blk_cnt))) return rc;   // per tile
    if ((rc = pv_get(ctx, "sum.tile_g0", (size_t)a.n_tiles + 2, &a.tile_g0))) return rc;
    if ((rc = pv_get(ctx, "sum.site_col", max_sites, &a.site_col))) return rc;
    if ((rc = pv_get(ctx, "sum.site_hdr", max_sites, &a.site_hdr))) return rc;
    if ((rc = pv_get(ctx, "sum.big_sites", max_sites, &a.big_sites))) return rc;
    if ((rc = pv_get(ctx, "sum.site_region", max_sites, &a.site_region))) return rc;
    if ((rc = pv_get(ctx, "sum.site_nev", max_sites, &a.site_nev))) return rc;
    if ((rc = pv_get(ctx, "sum.site_evoff", max_sites, &a.site_evoff))) return rc;
    if ((rc = pv_get(ctx, "sum.site_fill", max_sites, &a.site_fill))) return rc;
    if ((rc = pv_get(ctx, "sum.site_nemit", max_sites, &a.site_nemit))) return rc;
    if ((rc = pv_get(ctx, "sum.site_strbytes", max_sites, &a.site_strbytes))) return rc;
    if ((rc = pv_get(ctx, "sum.site_outoff", max_sites, &a.site_outoff))) return rc;
    if ((rc = pv_get(ctx, "sum.site_stroff", max_sites, &a.site_stroff))) return rc;
    if ((rc = pv_get(ctx, "sum.ev", max_events, &a.ev))) return rc;
    if ((rc = pv_get(ctx, "sum.rec", max_events + 4 * max_sites, &a.rec))) return rc;

    pv_prof_scope ps_all(ctx, "summary_pipeline", st);
    front_init(a, st);
    front_check_depth(a, st);
    front_pairs(ctx, a, st);
    { pv_prof_scope ps(ctx, "k_pileup", st); launch_pileup_tiles(a, hp, st); }
    k_site_rank<<<(unsigned)n_blk, 1024, 0, st>>>(a);
    k_scan_events<<<scan_chunks(a.max_sites), 1024, 0, st>>>(a);
    // per-site kernels are chains of dependent loads per wave: as many workgroups as can be resident (one site each for the
    // benchmark's ~8 k sites per launch)
    // (swept in round 2, 2048 .. 32768 workgroups: k_collect and k_write_windows are flat from 4096 / 8192 up, k_site_alleles
    // gains 5 us at 16384)
    const unsigned site_grid = (unsigned)(max_sites < 16384 ? (max_sites > 0 ? (max_sites + 7) / 8 * 8 : 8) : 16384);   // multiples of 8: xcd_site()
    const unsigned collect_grid = site_grid < 4096 ? site_grid : 4096;
    const unsigned ww_grid = site_grid < 8192 ? site_grid : 8192;
    if (n_cigar > 0 && n_reads > 0) { pv_prof_scope ps(ctx, "k_collect", st); k_collect<<<collect_grid, 64 * KC_WAVES, 0, st>>>(a); }
    {
        pv_prof_scope ps(ctx, "k_site_alleles", st);
        const unsigned big_grid = site_grid < 1024 ? site_grid : 1024;
        if (hp) {
            k_site_alleles<true, UM_SMALL, false><<<site_grid, 64, 0, st>>>(a);
            k_site_alleles<true, UMAX, true><<<big_grid, 64, 0, st>>>(a);
        } else {
            k_site_alleles<false, UM_SMALL, false><<<site_grid, 64, 0, st>>>(a);
            k_site_alleles<false, UMAX, true><<<big_grid, 64, 0, st>>>(a);
        }
    }
    k_scan_outputs<<<scan_chunks(a.max_sites), 1024, 0, st>>>(a);
    {
        pv_prof_scope ps(ctx, "k_write_windows", st);
        if (hp) k_write_windows<true><<<ww_grid, WW_THREADS, 0, st>>>(a);
        else k_write_windows<false><<<ww_grid, WW_THREADS, 0, st>>>(a);
    }
    PV_HIP(hipGetLastError());
    return PV_OK;
}

void default_limits(int64_t n_cols, int64_t n_cigar, int64_t n_bases, int64_t n_reads, int64_t capacity, bool hp,
                    int64_t* max_sites, int64_t* max_events, int64_t* max_pairs) {
    // a read touches span/TILE_COLS + 2 tiles at most and its in-region span is bounded by its aligned
    // bases plus deleted columns; deletions are rare, so allow 2x and let the device report overflow
    *max_pairs = 2 * (n_bases / TILE_COLS) + 3 * n_reads + 64;
    int64_t s = n_cols / 8 + 1024;
    if (s < 2 * capacity) s = 2 * capacity;
    if (s > n_cols) s = n_cols;
    if (s < 1) s = 1;
    *max_sites = s;
    *max_events = n_cigar + n_bases / 64 + 4096;
    if (hp) *max_events += n_bases / 16;  // every SNP observation at a site is an event in the haplotag form
}

}  // namespace pvsum

using namespace pvsum;

extern "C" int pv_summarize_regions_dev(pv_ctx* ctx, const pv_batch_in* in, const pv_params* params, int64_t n_reads,
                                        int64_t n_bases, int64_t n_cigar, int64_t n_ref_bytes, int64_t max_region_len,
                                        pv_batch_out* out, int64_t* d_counts, void* stream) {
    PV_CHECK(ctx && in && params && out && d_counts, PV_ERR_INVALID, "null argument");
    PV_CHECK(in->n_regions >= 0 && n_ref_bytes >= 0, PV_ERR_INVALID, "negative sizes");
    (void)max_region_len;
    PV_HIP(hipSetDevice(ctx->device));
    int64_t ms, me, mp;
    default_limits(n_ref_bytes, n_cigar, n_bases, n_reads, out->capacity, false, &ms, &me, &mp);
    return summarize_launch(ctx, in, params, n_reads, n_bases, n_cigar, n_ref_bytes > 0 ? n_ref_bytes : 1, ms, me, mp, out,
                            d_counts, pv_pick_stream(ctx, stream));
}

extern "C" int pv_summarize_regions_hp_dev(pv_ctx* ctx, const pv_batch_in* in, const int32_t* read_hp, const pv_params* params,
                                           int64_t n_reads, int64_t n_bases, int64_t n_cigar, int64_t n_ref_bytes,
                                           pv_batch_out* out, int64_t* d_counts, void* stream) {
    PV_CHECK(ctx && in && params && out && d_counts, PV_ERR_INVALID, "null argument");
    PV_CHECK(in->n_regions >= 0 && n_ref_bytes >= 0, PV_ERR_INVALID, "negative sizes");
    PV_HIP(hipSetDevice(ctx->device));
    int64_t ms, me, mp;
    default_limits(n_ref_bytes, n_cigar, n_bases, n_reads, out->capacity, true, &ms, &me, &mp);
    return summarize_launch(ctx, in, params, n_reads, n_bases, n_cigar, n_ref_bytes > 0 ? n_ref_bytes : 1, ms, me, mp, out,
                            d_counts, pv_pick_stream(ctx, stream), true, read_hp);
}
