// summary_pileup.hip — K2 of the image builders: the tile kernel that turns (read, tile) pairs into per-column counters and
// site flags, in its 26-plane and haplotag forms. summary_builder.hip launches it through launch_pileup_tiles().
#include "summary_launch.hpp"

namespace pvsum {
namespace {

// ---- K2 -------------------------------------------------------------------------------------------
// One workgroup per TILE of TILE_COLS columns. All 21 counters of the tile live in LDS for the whole
// kernel (ds_add instead of global atomics) and are written out once with coalesced stores, so the
// counter planes need no memset and see no global atomics.
// The tile's work is FLATTENED across the whole workgroup so that no latency chain is per read:
//   pair batch  : up to PT_PB (read, op-range) pair records -> LDS, block prefix sum of their op counts
//   op batch    : one THREAD per op over all pairs of the batch (512 ops at a time): CIGAR word, start
//                 column and read index are fetched with independent loads; indel bookkeeping per thread;
//                 block-wide prefix sum of the in-tile aligned-base counts
//   expansion   : the aligned bases of the 512 ops are dealt to the threads 4 consecutive bases at a
//                 time (one LDS binary search per 4 bases, all 12 byte loads issued before first use),
//                 so lanes stay busy whatever the CIGAR run lengths are and bytes are read coalesced.

// LDS counters of the tile kernel (all non-negative; converted to the global plane-major layout at
// flush time). The common case - a quality-passing A/C/G/T base over an A/C/G/T reference - costs ONE
// ds_add: coverage and the REFF/REFR planes are derived as sums (every counted base lands in exactly
// one symbol plane), anchors / odd symbols / non-ACGT reference columns use the side counters.
enum {
    L_P = 0,      // [2 strands][4]: base A,C,G,T counted over a valid reference
    L_X = 8,      // [2]: counted bases that are NOT in L_P (odd symbol, or reference not ACGT)
    L_O = 10,     // [2][3]: planes I, D, * (ops and odd symbols)
    L_ANC = 16,   // [2]: counted bases that anchor an indel (no REFF/REFR decrement, :381-391)
    L_COVI = 18,  // coverage bumps of the insert-anchor rule (:452-454)
    L_SNP = 19, L_INS = 20, L_DEL = 21, L_RARE = 22, L_N = 23
};

// LDS counters of the haplotag-aware form (region_summary_hp.cpp:393-463): a counted base costs TWO ds_adds whatever the
// read's tag is - one into its count-set class (coverage and the REF-count planes of both haplotypes are sums of classes),
// one into either the SNP counter or its symbol-set class (a match can only land in the plane of the reference's own symbol).
enum {
    HL_REFC = 0,   // [4 count-set classes: none, set 1, set 2, both][2 strands]: quality-passing aligned bases
    HL_M = 8,      // [3 symbol-set classes: set 1, set 2, both][2 strands]: bases equal to a valid reference base
    HL_O = 14,     // [2 sets][2 strands][3]: planes I, D, *
    HL_COVD = 26,  // coverage taken back by inserts that fail the quality bar (:487-488)
    HL_SNP = 27, HL_INS = 28, HL_DEL = 29, HL_N = 30
};

// Four bytes at a time: bit 7 of a result byte is set where the byte is NOT one of A/C/G/T (swar_not_acgt_upper) or not one of
// A/C/G/T/a/c/g/t (swar_not_acgt): two bits of the byte index a four-entry v_perm_b32 table of the expected letters, and what
// differs from it is non-zero
__device__ __forceinline__ uint32_t swar_nonzero(uint32_t z) { return (((z & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | z) & 0x80808080u; }
__device__ __forceinline__ uint32_t swar_not_acgt_upper(uint32_t w) {
    return swar_nonzero(__builtin_amdgcn_perm(0u, 0x47544341u, (w >> 1) & 0x03030303u) ^ w);   // index (b >> 1) & 3: A 0, C 1, T 2, G 3
}
__device__ __forceinline__ uint32_t swar_not_acgt(uint32_t w) { return swar_not_acgt_upper(w & 0xDFDFDFDFu); }

// Site flag of one column from its four counters: frequency thresholds of :634-646 (bit 0 site, bits 1-3 which of the
// SNP / insert / delete thresholds passed). Runs in the flush of k_pileup_tiles, where the counters still sit in LDS
// (it was a kernel of its own, k_site_scan, re-reading four planes: 16 us per 1.6 M columns, mostly round trips).
// A tile may run across region boundaries: the region of its first column is looked up when the workgroup starts
// (SiteRegion, off the tile's critical path), a column beyond it walks on from there.
struct SiteRegion { int g; int64_t off, next, R, start, cand_lo, cand_hi; };
__device__ __forceinline__ SiteRegion site_region_load(const SumArgs& a, int g) {
    SiteRegion r;
    r.g = g;
    const bool ok = g >= 0 && g < a.in.n_regions;
    r.off = ok ? a.in.ref_off[g] : 0;
    r.next = ok ? a.in.ref_off[g + 1] : 0;
    r.start = ok ? a.in.ref_start[g] : 0;
    r.R = ok ? a.in.ref_end[g] - r.start + 1 : 0;
    r.cand_lo = ok ? a.in.cand_start[g] : 1;
    r.cand_hi = ok ? a.in.cand_end[g] : 0;
    return r;
}
__device__ __forceinline__ uint8_t site_flag(const SumArgs& a, const SiteRegion& r0, int64_t col, int cov, int n_snp, int n_ins,
                                             int n_del) {
    SiteRegion r = r0;
    if (col >= r0.next) {  // (columns are >= the tile's first: only forwards)
        int g = r0.g;
        while (g + 1 <= a.in.n_regions && a.in.ref_off[g + 1] <= col) g++;
        r = site_region_load(a, g);
    }
    const int64_t i = col - r.off;
    if (i >= r.R) return 0;
    const double cv = (double)cov > 1.0 ? (double)cov : 1.0;
    const double fs = (double)n_snp / cv;
    const double fi = (double)n_ins / cv;
    const double fd = (double)n_del / cv;
    const bool ps = fs >= a.p.snp_freq_threshold, pi = fi >= a.p.insert_freq_threshold, pd = fd >= a.p.delete_freq_threshold;
    const int64_t pos = r.start + i;
    if ((ps || pi || pd) && pos >= r.cand_lo && pos <= r.cand_hi && (double)cov >= a.p.min_coverage_threshold)
        return (uint8_t)(1 | (ps ? 2 : 0) | (pi ? 4 : 0) | (pd ? 8 : 0));
    return 0;
}

template <bool HP>
__global__ __launch_bounds__(PT_THREADS, HP ? 2 : 4) void k_pileup_tiles(SumArgs a) {   // 26-plane form: two workgroups per CU (<= 128 VGPRs)
    __shared__ int32_t s_cnt[HP ? (int)HL_N : (int)L_N][TILE_COLS];
    __shared__ __attribute__((aligned(4))) uint8_t s_ref[TILE_COLS + 16];  // the tile's reference bytes (+16: groups of 4 / 8 columns are read as two / three aligned words from any column of the tile)
    __shared__ uint8_t s_lut[256];           // byte class: bits0-2 plane symbol 1..7, 8 = upper ACGT, 16 = lower acgt, 32 = valid reference
    constexpr int SB_N = 2048;               // 16-slot blocks with an owner entry (32 k slots per op batch; beyond: a search)
    __shared__ uint16_t s_blk[SB_N];         // op that owns the first slot of every 16-slot block: a padded op is ~12 slots, so the
                                             // walk from there is one step or none (64-slot blocks: two or three dependent reads)
    // per-op staging (one op batch)
    __shared__ int32_t s_pref[PT_THREADS];   // inclusive prefix of the in-tile aligned bases, every op padded to whole groups of 4
    // what the expansion needs of an op, as one 32-byte record (two ds_read_b128 per group instead of nine scalar reads):
    struct OpSt {
        int32_t i0s;     // i = j + i0s: offset in the op of slot j
        int32_t iend;    // one past the op's last in-tile base offset
        int32_t lcoff;   // tile-local column of op offset 0
        int32_t meta;    // len - 1
        int32_t base_lo, base_hi;  // global base index of op offset 0
        int32_t bleft;   // bases from there to the end of the read's sequence (saturated)
        int32_t fl;      // bit0 rev, bit1 anchor_next, haplotag form: bits 2-5
    };
    __shared__ __attribute__((aligned(16))) OpSt s_op[PT_THREADS];
    // per-pair staging (one pair batch)
    __shared__ int32_t p_off[PT_PB + 1];     // exclusive prefix of op counts
    constexpr int PB_BLK = 768;              // 32-op blocks of a pair batch with an owner entry (24 k ops; beyond: binary search)
    __shared__ uint8_t p_blk[PB_BLK];
    __shared__ int32_t p_oplo[PT_PB], p_colbase[PT_PB], p_R[PT_PB], p_clast[PT_PB], p_reflen[PT_PB], p_rev[PT_PB];
    __shared__ int64_t p_base0[PT_PB], p_seqend[PT_PB];
    __shared__ int32_t s_wsum[2 * (PT_THREADS / 64)];
    int scan_turn = 0;
    const int tid = threadIdx.x;
    const int64_t tile = blockIdx.x;
#ifdef PV_PSTAMPS
    unsigned long long ps_t0, ps_t1, ps_acc[6] = {0, 0, 0, 0, 0, 0};
#define PSTAMP(i) { asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(ps_t1) :: "memory"); ps_acc[i] += ps_t1 - ps_t0; ps_t0 = ps_t1; }
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(ps_t0) :: "memory");
#else
#define PSTAMP(i)
#endif
    const int64_t tlo = tile * TILE_COLS, thi = tlo + TILE_COLS - 1;  // global columns of this tile
    __shared__ SiteRegion s_sreg;  // region of the tile's first column, for the flush (looked up by k_init)
    if (tid == 0) s_sreg = site_region_load(a, a.tile_g0[tile]);
    for (int i = tid; i < (HP ? (int)HL_N : (int)L_N) * TILE_COLS; i += PT_THREADS) (&s_cnt[0][0])[i] = 0;
    for (int i = tid; i < TILE_COLS + 16; i += PT_THREADS) s_ref[i] = (i < TILE_COLS && tlo + i < a.n_cols) ? a.in.ref[tlo + i] : (uint8_t)'N';
    if (tid < 256) s_lut[tid] = (uint8_t)(sym_of(tid) | (is_acgt(tid) ? 8 : 0) | ((tid != up(tid) && is_acgt(up(tid))) ? 16 : 0) | (is_acgt(up(tid)) ? 32 : 0));
    const int32_t p0 = a.tile_off[tile];
    const int32_t np = a.tile_cnt[tile];
    // quality bar as a per-byte compare: q >= qmin  <=>  high bits decide, or are equal and the low seven bits decide
    [[maybe_unused]] const uint32_t q_low = (uint32_t)(a.qmin_snp & 0x7F) * 0x01010101u;
    [[maybe_unused]] const bool q_hi = a.qmin_snp >= 128, q_all = a.qmin_snp <= 0, q_none = a.qmin_snp > 255;
    __syncthreads();
    for (int32_t pb = 0; pb < np; pb += PT_PB) {
        const int npb = (np - pb) < PT_PB ? (np - pb) : PT_PB;
        // ---- pair batch -> LDS -----------------------------------------------------------------------
        int nops = 0;
        if (tid < npb) {
            const PairRec pr = a.pairs[p0 + pb + tid];
            nops = pr.op_hi - pr.op_lo;
            p_oplo[tid] = pr.op_lo; p_colbase[tid] = pr.col_base; p_R[tid] = pr.R; p_clast[tid] = pr.c_last;
            p_reflen[tid] = pr.ref_len; p_rev[tid] = pr.rev; p_base0[tid] = pr.base0; p_seqend[tid] = pr.seq_end;
        }
        const int incl_ops = block_incl_scan512(nops, s_wsum, tid, scan_turn);
        if (tid < npb) {
            p_off[tid + 1] = incl_ops;
            // pair that owns the first op of every 32-op block that starts inside this pair's range (op -> pair lookups start there)
            for (int bb = (incl_ops - nops + 31) >> 5; (bb << 5) < incl_ops && bb < PB_BLK; bb++) p_blk[bb] = (uint8_t)tid;
        }
        if (tid == 0) p_off[0] = 0;
        __syncthreads();
        const int total_ops = p_off[npb];
        PSTAMP(0)  // pair batch
        // the four words of an op (start column, CIGAR word, read offset, next CIGAR word) are requested one op batch AHEAD:
        // the batch's first phase is otherwise a chain of dependent round trips (pair lookup -> op words -> indel qualities)
        struct OpWords { int pslot; int32_t c, c_last, rr, rdv; uint32_t w, wn; };
        auto op_fetch = [&](int kk) {
            OpWords o;
            o.pslot = 0; o.c = 0; o.c_last = 0; o.rr = OP_INACTIVE; o.rdv = 0; o.w = 15u; o.wn = 15u;
            if (kk < total_ops) {
                int lo;  // last pair slot with p_off[slot] <= kk: the owner of the op's 32-op block, then a short walk
                if ((kk >> 5) < PB_BLK) {
                    lo = p_blk[kk >> 5];
                    while (p_off[lo + 1] <= kk) lo++;
                } else {
                    int hi = npb;
                    lo = 0;
                    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (p_off[mid] <= kk) lo = mid; else hi = mid; }
                }
                o.pslot = lo;
                o.c = p_oplo[lo] + (kk - p_off[lo]);
                o.c_last = p_clast[lo];
                o.rr = a.op_ref[o.c];
                o.w = a.in.cigar[o.c];
                o.rdv = a.op_rd[o.c];
                o.wn = a.in.cigar[o.c < o.c_last ? o.c + 1 : o.c];
            }
            return o;
        };
        OpWords ow_next = op_fetch(tid);
        for (int ob = 0; ob < total_ops; ob += PT_THREADS) {
            // ---- op batch: one thread per op -----------------------------------------------------------
            const int k = ob + tid;
            int32_t ref_rel = 0, rd = 0, len = 0, op = 15, col_base = 0;
            bool active = false, anchor_next = false, rev = false;
            int pslot = 0, hpbits = 0;  // hpbits: bits 0-1 count sets, bits 2-3 symbol sets (haplotag form only)
            int32_t c = 0;
            int64_t clo = 0, chi = -1;
            const OpWords ow = ow_next;
            if (k < total_ops) {
                pslot = ow.pslot;
                c = ow.c;
                const int32_t c_last = ow.c_last;
                const int32_t rr = ow.rr;
                const uint32_t w = ow.w;
                const int32_t rdv = ow.rdv;
                const uint32_t wn = ow.wn;
                col_base = p_colbase[pslot];
                rev = (p_rev[pslot] & 1) != 0;
                hpbits = p_rev[pslot] >> 1;
                active = rr != OP_INACTIVE;
                if (active) {
                    ref_rel = rr; rd = rdv; op = w & 0xF; len = (int32_t)(w >> 4);
                    const int nop = wn & 0xF;
                    anchor_next = (c < c_last) && (nop == PV_CIGAR_IN || nop == PV_CIGAR_DEL);  // :381-391
                }
                clo = tlo - col_base; chi = thi - col_base;  // tile columns relative to the region, clipped to it
                if (clo < 0) clo = 0;
                if (chi > p_R[pslot] - 1) chi = p_R[pslot] - 1;
            }
            [[maybe_unused]] const int so = L_O + (rev ? 3 : 0);
            // (0) an insert anchored in this tile: the qualities of its anchor base and its inserted bases (bytes [start, start + L),
            // start = the base before the insert, L = len + 1) are REQUESTED here and - haplotag form - used behind the scans and the
            // staging below: the one HBM round trip of this phase that nothing used to cover
            bool ins_here = false, ins_long = false;   // (start and column are recomputed when used: the kernel sits at its register cap)
            uint32_t ins_qlo = 0, ins_qhi = 0;
            if (active && op == PV_CIGAR_IN) {  // region_summary.cpp:431-490 / region_summary_hp.cpp:469-553
                const int64_t anchor = (int64_t)ref_rel - 1;
                if (anchor >= clo && anchor <= chi && rd >= 1) {
                    const int64_t ins_start = p_base0[pslot] + rd - 1;
                    const int64_t L = (int64_t)len + 1;
                    if (ins_start + L > p_seqend[pslot]) {
                        set_status(a.diag, PV_ERR_INVALID);
                    } else {
                        ins_here = true;
                        if (L <= 8 && ins_start + 8 <= a.n_bases) {  // the usual short insert: ONE round trip instead of L dependent ones
                            ins_qlo = *reinterpret_cast<const uint32_t*>(a.in.quals + ins_start);
                            ins_qhi = *reinterpret_cast<const uint32_t*>(a.in.quals + ins_start + 4);
                        } else {
                            ins_long = true;
                        }
                    }
                }
            }
            auto ins_use = [&]() {
                if (!ins_here) return;
                const int64_t L = (int64_t)len + 1;
                int64_t qs_all = 0;   // anchor base + inserted bases
                int q0;               // the anchor base
                if (!ins_long) {
                    uint32_t lo = ins_qlo, hi = ins_qhi;
                    if (L <= 4) { hi = 0; if (L < 4) lo &= (1u << (8 * (int)L)) - 1u; }
                    else if (L < 8) hi &= (1u << (8 * ((int)L - 4))) - 1u;
                    q0 = (int)(lo & 0xFF);
                    qs_all = (int64_t)__builtin_amdgcn_sad_u8(lo, 0u, __builtin_amdgcn_sad_u8(hi, 0u, 0u));
                } else {
                    const int64_t ins_start = p_base0[pslot] + rd - 1;
                    for (int64_t i = 0; i < L; i++) qs_all += a.in.quals[ins_start + i];
                    q0 = a.in.quals[ins_start];
                }
                const int lc = (int)((int64_t)col_base + ref_rel - 1 - tlo);
                if constexpr (HP) {
                    const int st = rev ? 1 : 0, ss = hpbits >> 2;
                    const bool qok = (double)(qs_all - q0) >= a.p.min_indel_baseq * (double)len;   // inserted bases only, :482-484
                    if (!qok && (double)q0 >= a.p.min_snp_baseq) atomicAdd(&s_cnt[HL_COVD][SW(lc)], 1);
                    if (2 + (int64_t)len <= PV_MAX_ALLELE_KEY && qok) {
                        if (is_acgt(up(s_ref[lc]))) {
                            if (ss & 1) atomicAdd(&s_cnt[HL_O + (0 + st) * 3 + 0][SW(lc)], 1);
                            if (ss & 2) atomicAdd(&s_cnt[HL_O + (2 + st) * 3 + 0][SW(lc)], 1);
                        }
                        atomicAdd(&s_cnt[HL_INS][SW(lc)], 1);
                    }
                } else {
                    const bool qok = (double)qs_all >= a.p.min_indel_baseq * (double)L;
                    if (qok && (double)q0 < a.p.min_snp_baseq) atomicAdd(&s_cnt[L_COVI][SW(lc)], 1);  // :453
                    if (1 + L <= PV_MAX_ALLELE_KEY && qok) {
                        if (is_acgt(up(s_ref[lc]))) atomicAdd(&s_cnt[so + 0][SW(lc)], 1);
                        atomicAdd(&s_cnt[L_INS][SW(lc)], 1);
                    }
                }
            };
            // The 26-plane form sits at its 128-register cap (two more live values spill): it uses the words at once, as before;
            // the haplotag form (one workgroup per CU, 256 registers) uses them behind the scans.
            // the next batch's op words are requested BEHIND the insert's qualities (so that waiting for those leaves these in
            // flight) and ahead of the delete bookkeeping, which is LDS work: its time and the pair lookup of the prefetch cover
            // most of the qualities' round trip before the 26-plane form uses them
            if (ob + PT_THREADS < total_ops) ow_next = op_fetch(k + PT_THREADS);
            // (1) delete ops; an op belongs to the tile that owns its anchor column
            if constexpr (HP) {
                const int st = rev ? 1 : 0, ss = hpbits >> 2;
                if (active && op == PV_CIGAR_DEL) {  // :556-649
                    const int64_t anchor = (int64_t)ref_rel - 1;
                    if (anchor >= clo && anchor <= chi) {
                        const int lc = (int)(col_base + anchor - tlo);
                        if (is_acgt(up(s_ref[lc]))) {  // unconditional, :561-569
                            if (ss & 1) atomicAdd(&s_cnt[HL_O + (0 + st) * 3 + 1][SW(lc)], 1);
                            if (ss & 2) atomicAdd(&s_cnt[HL_O + (2 + st) * 3 + 1][SW(lc)], 1);
                        }
                        int64_t L = (int64_t)len + 1;
                        if (anchor + L > p_reflen[pslot]) L = p_reflen[pslot] - anchor;
                        if (1 + L <= PV_MAX_ALLELE_KEY) {
                            atomicAdd(&s_cnt[HL_DEL][SW(lc)], 1);
                            }
                    }
                    int64_t i0 = clo - ref_rel; if (i0 < 0) i0 = 0;
                    int64_t i1 = chi + 1 - ref_rel; if (i1 > len) i1 = len;
                    for (int64_t i = i0; i < i1; i += 8) {  // :631-647, eight deleted columns per pass (see the 26-plane form)
                        const int lcb = (int)((int64_t)col_base + ref_rel + i - tlo);
                        const int n = (int)(i1 - i < 8 ? i1 - i : 8);
                        const uint32_t* wp = reinterpret_cast<const uint32_t*>(s_ref) + (lcb >> 2);
                        const uint32_t w0 = wp[0], w1 = wp[1], w2 = wp[2];
                        const uint32_t bad0 = swar_not_acgt(__builtin_amdgcn_alignbyte(w1, w0, (unsigned)lcb & 3u));
                        const uint32_t bad1 = swar_not_acgt(__builtin_amdgcn_alignbyte(w2, w1, (unsigned)lcb & 3u));
#pragma unroll
                        for (int e = 0; e < 8; e++) {
                            const int inc = e < n ? (int)((((e < 4 ? bad0 : bad1) >> (8 * (e & 3) + 7)) & 1u) ^ 1u) : 0;
                            const int sw = SW(lcb + e);
                            atomicAdd(&s_cnt[HL_O + (0 + st) * 3 + 2][sw], (ss & 1) ? inc : 0);
                            atomicAdd(&s_cnt[HL_O + (2 + st) * 3 + 2][sw], (ss & 2) ? inc : 0);
                        }
                    }
                }
            } else {
            if (active && op == PV_CIGAR_DEL) {  // :491-555
                const int64_t anchor = (int64_t)ref_rel - 1;
                if (anchor >= clo && anchor <= chi) {
                    const int lc = (int)(col_base + anchor - tlo);
                    if (is_acgt(up(s_ref[lc]))) atomicAdd(&s_cnt[so + 1][SW(lc)], 1);  // unconditional, :496
                    int64_t L = (int64_t)len + 1;
                    if (anchor + L > p_reflen[pslot]) L = p_reflen[pslot] - anchor;  // substr truncation, :500
                    if (1 + L <= PV_MAX_ALLELE_KEY) {
                        atomicAdd(&s_cnt[L_DEL][SW(lc)], 1);
                    }
                }
                int64_t i0 = clo - ref_rel; if (i0 < 0) i0 = 0;
                int64_t i1 = chi + 1 - ref_rel; if (i1 > len) i1 = len;
                // :542-552, the '*' plane of the deleted columns inside the tile where the reference is A/C/G/T. Eight columns per
                // pass: their reference bytes arrive as three aligned words and are tested together, and the adds (ZERO where a
                // column does not count; SW() keeps any column inside the plane) follow each other with no read between them -
                // a column at a time was a chain of dependent LDS round trips, the longest part of this phase
                for (int64_t i = i0; i < i1; i += 8) {
                    const int lcb = (int)((int64_t)col_base + ref_rel + i - tlo);
                    const int n = (int)(i1 - i < 8 ? i1 - i : 8);
                    const uint32_t* wp = reinterpret_cast<const uint32_t*>(s_ref) + (lcb >> 2);
                    const uint32_t w0 = wp[0], w1 = wp[1], w2 = wp[2];
                    const uint32_t bad0 = swar_not_acgt(__builtin_amdgcn_alignbyte(w1, w0, (unsigned)lcb & 3u));
                    const uint32_t bad1 = swar_not_acgt(__builtin_amdgcn_alignbyte(w2, w1, (unsigned)lcb & 3u));
#pragma unroll
                    for (int e = 0; e < 8; e++) {
                        const int inc = e < n ? (int)((((e < 4 ? bad0 : bad1) >> (8 * (e & 3) + 7)) & 1u) ^ 1u) : 0;
                        atomicAdd(&s_cnt[so + 2][SW(lcb + e)], inc);
                    }
                }
            }
            }
            if constexpr (!HP) ins_use();
            // (2) aligned bases of the batch's M/=/X ops, clipped to tile and region
            PSTAMP(1)  // op lookup + indel ops
            const bool is_m = active && (op == PV_CIGAR_MATCH || op == PV_CIGAR_EQUAL || op == PV_CIGAR_DIFF);
            int32_t i0 = 0, eff = 0;
            if (is_m) {
                int64_t lo = clo - ref_rel; if (lo < 0) lo = 0;
                int64_t hi = chi + 1 - ref_rel; if (hi > len) hi = len;
                if (hi > lo) { i0 = (int32_t)lo; eff = (int32_t)(hi - lo); }
            }
            // Slots: every op's in-tile bases are padded to whole groups of 4 slots, so that a GROUP never straddles two ops:
            // one owner lookup, one dword load of bases and one of qualities serve 4 consecutive bases / columns.
            const int32_t effp = (eff + 3) & ~3;
            const int32_t incl = block_incl_scan512(effp, s_wsum, tid, scan_turn);
            s_pref[tid] = incl;
            {
                const int64_t base = (k < total_ops ? p_base0[pslot] : 0) + rd;
                int64_t bleft = (k < total_ops ? p_seqend[pslot] : 0) - base;
                bleft = bleft > 0x7fffffff ? 0x7fffffff : (bleft < -0x7fffffff ? -0x7fffffff : bleft);
                OpSt o;
                o.i0s = i0 - (incl - effp);
                o.iend = i0 + eff;
                o.lcoff = (int32_t)((int64_t)col_base + ref_rel - tlo);
                o.meta = len - 1;
                o.base_lo = (int32_t)(uint32_t)base;
                o.base_hi = (int32_t)(base >> 32);
                o.bleft = (int32_t)bleft;
                o.fl = (rev ? 1 : 0) | (anchor_next ? 2 : 0) | (HP ? hpbits << 2 : 0);
                s_op[tid] = o;
            }
            for (int32_t bb = (incl - effp + 15) >> 4; (bb << 4) < incl && bb < SB_N; bb++) s_blk[bb] = (uint16_t)tid;  // blocks starting inside this op
            __syncthreads();
            const int32_t total = s_pref[PT_THREADS - 1];
            if constexpr (HP) ins_use();   // (0, continued) the insert's qualities have arrived by now
            PSTAMP(2)  // scan + staging + barrier
            // ---- expansion: PT_GPL groups of 4 consecutive bases per thread per trip; the owner lookups and the loads of
            // trip t+1 are issued before trip t is counted, so the HBM round trip of the bases hides behind the ds_adds ----
            struct Grp { int lc, nv, fl, last; uint32_t bw, qw, rw; };
            auto look = [&](int32_t jb, Grp (&g)[PT_GPL]) {
#pragma unroll
                for (int u = 0; u < PT_GPL; u++) {
                    // consecutive lanes take consecutive groups: the dword loads of a wave cover 256 consecutive bytes of a run
                    const int32_t j = jb + (u * PT_THREADS + tid) * 4;
                    const bool ok = j < total;
                    int owc = 0;                       // owner of the block's first slot, then a short probe
                    if (ok) {
                        if ((j >> 4) < SB_N) {
                            owc = s_blk[j >> 4];
                        } else {                       // first op whose inclusive prefix exceeds j
                            int hi = PT_THREADS - 1;
                            while (owc < hi) { const int mid = (owc + hi) >> 1; if (s_pref[mid] <= j) owc = mid + 1; else hi = mid; }
                        }
                        while (s_pref[owc] <= j) owc++;
                    }
                    const OpSt o = s_op[owc];
                    const int32_t i = j + o.i0s;
                    int nv = o.iend - i;               // valid bases of the group (the rest is padding)
                    nv = ok ? (nv > 4 ? 4 : nv) : 0;
                    const int64_t bi = (int64_t)(((uint64_t)(uint32_t)o.base_hi << 32) | (uint32_t)o.base_lo) + i;
                    const int64_t left = (int64_t)o.bleft - i;
                    if (nv > 0 && nv > left) { set_status(a.diag, PV_ERR_INVALID); nv = left > 0 ? (int)left : 0; }
                    const int lc = o.lcoff + i;
                    g[u].lc = lc;
                    g[u].nv = nv;
                    const int f = o.fl;
                    g[u].fl = HP ? f : (f & 1);
                    g[u].last = (f & 2) ? o.meta - i : -1;  // group position of the op's last base, if that base anchors an indel
                    uint32_t b4 = 0, q4 = 0;
                    if (nv > 0) {
                        if (bi + 4 <= a.n_bases) {  // unaligned dword loads
                            b4 = *reinterpret_cast<const uint32_t*>(a.in.bases + bi);
                            q4 = *reinterpret_cast<const uint32_t*>(a.in.quals + bi);
                        } else {
                            for (int e = 0; e < nv; e++) {
                                b4 |= (uint32_t)a.in.bases[bi + e] << (8 * e);
                                q4 |= (uint32_t)a.in.quals[bi + e] << (8 * e);
                            }
                        }
                    }
                    g[u].bw = b4; g[u].qw = q4;
                    const int lcr = nv > 0 ? lc : 0;   // four reference bytes from lcr on: two aligned words, shifted together
                    const uint32_t* rwp = reinterpret_cast<const uint32_t*>(s_ref) + (lcr >> 2);
                    g[u].rw = __builtin_amdgcn_alignbyte(rwp[1], rwp[0], (unsigned)lcr & 3u);
                }
            };
            // general classification of one counted base (any byte over any reference byte), :379-423
            auto count_general = [&](const Grp& G, int e, int st) {
                const int base = (G.bw >> (8 * e)) & 0xFF, refb = (G.rw >> (8 * e)) & 0xFF;
                const int lc = G.lc + e;
                const int cb = s_lut[base];
                const bool refvalid = (s_lut[refb] & 32) != 0;
                const int sy = cb & 7;                                           // 1..7
                if (refvalid && sy <= 4) {
                    atomicAdd(&s_cnt[L_P + 4 * st + (sy - 1)][SW(lc)], 1);       // :379 + :381-391 + :396,423 in one
                } else {
                    atomicAdd(&s_cnt[L_X + st][SW(lc)], 1);
                    if (refvalid) atomicAdd(&s_cnt[L_O + 3 * st + (sy - 5)][SW(lc)], 1);
                }
                if (e == G.last) atomicAdd(&s_cnt[L_ANC + st][SW(lc)], 1);
                const bool mism = refb != base;                                  // raw bytes, :394
                if (mism) atomicAdd(&s_cnt[L_SNP][SW(lc)], 1);
                const bool rare = mism && !(refvalid && (cb & 8));
                const bool corr = refvalid && (cb & 16);
                if (rare || corr) atomicAdd(&s_cnt[L_RARE][SW(lc)], 1);
            };
            auto count = [&](const Grp (&g)[PT_GPL]) {
#pragma unroll
                for (int u = 0; u < PT_GPL; u++) {
                    // quality bar and the group's valid bases, a byte per base (bit 7 = counts)
                    constexpr uint32_t H = 0x80808080u;
                    const Grp& G = g[u];
                    const uint32_t tq = (G.qw | H) - q_low;                              // bit 7: low seven bits of q >= those of qmin
                    uint32_t ge = q_hi ? (G.qw & tq) : (G.qw | tq);
                    ge = q_all ? H : (q_none ? 0u : ge);
                    const uint32_t vm = G.nv >= 4 ? H : ((H >> 8) >> (24 - 8 * (G.nv < 0 ? 0 : G.nv)));   // the group's valid bases
                    const uint32_t ok = ge & vm;
                    if constexpr (HP) {  // region_summary_hp.cpp:393-463: a counted base adds to its count-set class and to either the
                        // SNP counter (raw bytes differ, :406) or - over a valid reference - its symbol-set class; branch-free like the
                        // 26-plane form (a base that does not count adds zero)
                        const uint32_t differs = swar_nonzero(G.bw ^ G.rw);
                        const uint32_t second = ok & (differs | ~swar_not_acgt(G.rw));
                        const int st = G.fl & 1, cs = (G.fl >> 2) & 3, ss = (G.fl >> 4) & 3;
#pragma unroll
                        for (int e = 0; e < 4; e++) {
                            const int sw = SW(G.lc + e);
                            atomicAdd(&s_cnt[HL_REFC + 2 * cs + st][sw], (int)((ok >> (8 * e + 7)) & 1u));
                            const bool mm = ((differs >> (8 * e + 7)) & 1u) != 0;
                            atomicAdd(&s_cnt[mm ? (int)HL_SNP : HL_M + 2 * (ss - 1) + st][sw], (int)((second >> (8 * e + 7)) & 1u));
                        }
                    } else {
                        // The four bases of a group are classified together, a byte per base in 32-bit operations (bit 7 of a byte =
                        // the answer for that base), so that the usual base - A/C/G/T in upper case over an A/C/G/T reference of
                        // either case, quality passing - costs a bit test, an address and its one ds_add; bases that are anything
                        // else take count_general, one by one.
                        const uint32_t selb = (G.bw >> 1) & 0x03030303u;                     // A 0, C 1, T 2, G 3
                        const uint32_t b_bad = swar_not_acgt_upper(G.bw);
                        const uint32_t r_bad = swar_not_acgt(G.rw);
                        const uint32_t fast = ok & ~(b_bad | r_bad);
                        const uint32_t slow = ok & (b_bad | r_bad);
                        const uint32_t mism = swar_nonzero(G.bw ^ G.rw) & fast;                   // raw bytes, :394 (never rare: both are A/C/G/T)
                        const uint32_t pidx = selb ^ ((selb >> 1) & 0x01010101u);            // -> A 0, C 1, G 2, T 3
                        const int st = G.fl;
                        // no branches: a base that does not count adds ZERO (SW() keeps any column inside the plane, the plane
                        // index is two bits of the byte), which costs the LDS nothing it was not already doing - some lane of
                        // the wave nearly always counts - and saves the exec-mask bookkeeping per base
#pragma unroll
                        for (int e = 0; e < 4; e++) {
                            const int sw = SW(G.lc + e);
                            atomicAdd(&s_cnt[L_P + 4 * st + (int)((pidx >> (8 * e)) & 3u)][sw], (int)((fast >> (8 * e + 7)) & 1u));
                            atomicAdd(&s_cnt[L_SNP][sw], (int)((mism >> (8 * e + 7)) & 1u));
                        }
                        {
                            const unsigned la = (unsigned)G.last < 4u ? (unsigned)G.last : 0u;
                            const int inc = (unsigned)G.last < 4u ? (int)((fast >> (8 * la + 7)) & 1u) : 0;
                            atomicAdd(&s_cnt[L_ANC + st][SW(G.lc + (int)la)], inc);
                        }
                        if (slow) {
#pragma unroll
                            for (int e = 0; e < 4; e++)
                                if (slow & (0x80u << (8 * e))) count_general(G, e, st);
                        }
                    }
                }
            };
            constexpr int32_t TRIP = PT_THREADS * PT_GPL * 4;
            Grp ga[PT_GPL], gb[PT_GPL];
            if (total > 0) look(0, ga);
            for (int32_t jb = 0; jb < total; jb += 2 * TRIP) {
                if (jb + TRIP < total) look(jb + TRIP, gb);
                count(ga);
                if (jb + TRIP < total) {
                    if (jb + 2 * TRIP < total) look(jb + 2 * TRIP, ga);
                    count(gb);
                }
            }
            PSTAMP(3)  // expansion
            __syncthreads();  // staging arrays are rewritten by the next op batch
            PSTAMP(4)
        }
        __syncthreads();  // pair arrays are rewritten by the next pair batch
    }
    __syncthreads();
    // flush: derive the global plane-major counters (negative counts, as the reference keeps them)
    PSTAMP(4)
    const int64_t NC = a.n_cols;
    int64_t ncol = NC - tlo;
    if (ncol > TILE_COLS) ncol = TILE_COLS;
    static_assert(TILE_COLS <= PT_THREADS, "one column per thread: the site count below is a ballot");
    int site = 0;
    const SiteRegion sreg = s_sreg;
    // Pass 1: the four site counters of this thread's column, its flag, and - a ballot per wave - which columns of the tile are
    // sites. Pass 2 writes the counter planes ONLY where something will read them: the planes are read at site columns
    // (k_site_rank, k_site_alleles) and in the windows around them (k_write_windows: W columns to either side), i.e. ~20 % of the
    // columns at one site per ~190 columns; a column within W of the tile's edge is written anyway, because the site that needs it
    // may lie in the next tile. (Before: every column of every plane, 85 MB per 16 regions, the largest write of the chain.)
    constexpr int W = HP ? (PV_HP_WINDOW_ROWS - 1) / 2 : (PV_WINDOW_ROWS - 1) / 2;
    __shared__ unsigned long long s_sitebits[PT_THREADS / 64];
    int cov = 0, n_snp = 0, n_ins = 0, n_del = 0;
    const int lc = tid;                      // one column per thread (TILE_COLS == PT_THREADS)
    const bool have = lc < ncol;
    const int64_t g = tlo + lc;
    if (have) {
        if constexpr (HP) {
            cov = -s_cnt[HL_COVD][SW(lc)];
#pragma unroll
            for (int k = 0; k < 8; k++) cov += s_cnt[HL_REFC + k][SW(lc)];
            n_snp = s_cnt[HL_SNP][SW(lc)]; n_ins = s_cnt[HL_INS][SW(lc)]; n_del = s_cnt[HL_DEL][SW(lc)];
        } else {
            cov = s_cnt[L_COVI][SW(lc)];
#pragma unroll
            for (int st = 0; st < 2; st++) {
#pragma unroll
                for (int k = 0; k < 4; k++) cov += s_cnt[L_P + 4 * st + k][SW(lc)];
                cov += s_cnt[L_X + st][SW(lc)];
            }
            n_snp = s_cnt[L_SNP][SW(lc)]; n_ins = s_cnt[L_INS][SW(lc)]; n_del = s_cnt[L_DEL][SW(lc)];
        }
        const uint8_t f = site_flag(a, sreg, g, cov, n_snp, n_ins, n_del);
        a.flags[g] = f;
        site = f & 1;
    }
    const unsigned long long site_m = __ballot(site);
    if ((tid & 63) == 0) s_sitebits[tid >> 6] = site_m;
    __syncthreads();
    bool need = have && (lc < W || lc >= (int)ncol - W);
    if (have && !need) {
        const int c0 = lc - W, c1 = lc + W;   // inside [0, ncol) here
#pragma unroll
        for (int wdx = 0; wdx < PT_THREADS / 64; wdx++) {
            const int lo = wdx * 64, hi = lo + 63;
            if (c1 < lo || c0 > hi) continue;
            const int b0_ = c0 > lo ? c0 - lo : 0, b1_ = c1 < hi ? c1 - lo : 63;
            const unsigned long long mask = (b1_ - b0_ == 63) ? ~0ull : (((1ull << (b1_ - b0_ + 1)) - 1ull) << b0_);
            need = need || (s_sitebits[wdx] & mask) != 0;
        }
    }
    if (need) {
        if constexpr (HP) {
            cnt_t v[CNT_STRIDE_HP];
#pragma unroll
            for (int k = 0; k < CNT_STRIDE_HP; k++) v[k] = 0;
            const int rsym = s_lut[s_ref[lc]];  // bits0-2: plane symbol of the reference byte, bit 5: valid reference
#pragma unroll
            for (int set = 0; set < 2; set++) {
#pragma unroll
                for (int st = 0; st < 2; st++) {
                    const int grp = 2 * set + st;
                    cnt_t* dst = v + HC_PLANE + 8 * grp;
                    dst[0] = (cnt_t)-(s_cnt[HL_REFC + 2 * (1 + set) + st][SW(lc)] + s_cnt[HL_REFC + 2 * 3 + st][SW(lc)]);
                    const int m = s_cnt[HL_M + 2 * set + st][SW(lc)] + s_cnt[HL_M + 2 * 2 + st][SW(lc)];
#pragma unroll
                    for (int k = 0; k < 4; k++) dst[1 + k] = (cnt_t)(((rsym & 32) && (rsym & 7) == k + 1) ? -m : 0);
#pragma unroll
                    for (int k = 0; k < 3; k++) dst[5 + k] = (cnt_t)s_cnt[HL_O + grp * 3 + k][SW(lc)];
                }
            }
            v[C_COV] = (cnt_t)cov; v[C_SNP] = (cnt_t)n_snp; v[C_INS] = (cnt_t)n_ins; v[C_DEL] = (cnt_t)n_del;
            cnt_u32x4* dst4 = reinterpret_cast<cnt_u32x4*>(a.cnt + g * CNT_STRIDE_HP);
#pragma unroll
            for (int k = 0; k < CNT_STRIDE_HP / 8; k++) {
                cnt_u32x4 w4;
#pragma unroll
                for (int j = 0; j < 4; j++) w4[j] = (uint32_t)(uint16_t)v[8 * k + 2 * j] | ((uint32_t)(uint16_t)v[8 * k + 2 * j + 1] << 16);
                dst4[k] = w4;
            }
        } else {
            cnt_t v[CNT_STRIDE];
#pragma unroll
            for (int k = 0; k < CNT_STRIDE; k++) v[k] = 0;
#pragma unroll
            for (int st = 0; st < 2; st++) {
                int sp = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int x = s_cnt[L_P + 4 * st + k][SW(lc)];
                    sp += x;
                    v[C_PLANE + 8 * st + 1 + k] = (cnt_t)-x;
                }
                const int counted = sp + s_cnt[L_X + st][SW(lc)];
                v[C_PLANE + 8 * st] = (cnt_t)-(counted - s_cnt[L_ANC + st][SW(lc)]);
#pragma unroll
                for (int k = 0; k < 3; k++) v[C_PLANE + 8 * st + 5 + k] = (cnt_t)-s_cnt[L_O + 3 * st + k][SW(lc)];
            }
            v[C_COV] = (cnt_t)cov; v[C_SNP] = (cnt_t)n_snp; v[C_INS] = (cnt_t)n_ins; v[C_DEL] = (cnt_t)n_del;
            v[C_RARE] = (cnt_t)s_cnt[L_RARE][SW(lc)];
            cnt_u32x4* dst4 = reinterpret_cast<cnt_u32x4*>(a.cnt + g * CNT_STRIDE);
#pragma unroll
            for (int k = 0; k < CNT_STRIDE / 8; k++) {
                cnt_u32x4 w4;
#pragma unroll
                for (int j = 0; j < 4; j++) w4[j] = (uint32_t)(uint16_t)v[8 * k + 2 * j] | ((uint32_t)(uint16_t)v[8 * k + 2 * j + 1] << 16);
                dst4[k] = w4;
            }
        }
    }
    if ((tid & 63) == 0 && site_m) atomicAdd(&a.blk_cnt[tile], __popcll(site_m));
#ifdef PV_PSTAMPS
    PSTAMP(5)  // flush
    if (tid == 0 && a.site_strbytes) {  // debug: reuse a workspace array that is written later in the pipeline
        for (int i = 0; i < 6; i++) atomicAdd((unsigned long long*)&a.diag[D_NDIAG + i], ps_acc[i]);
    }
#endif
#undef PSTAMP
}

}  // namespace

void launch_pileup_tiles(const SumArgs& a, bool hp, hipStream_t st) {
    if (hp) k_pileup_tiles<true><<<(unsigned)a.n_tiles, PT_THREADS, 0, st>>>(a);
    else k_pileup_tiles<false><<<(unsigned)a.n_tiles, PT_THREADS, 0, st>>>(a);
}

}  // namespace pvsum

#ifdef PV_PSTAMPS
// diagnostic builds only: phase cycle sums of the last k_pileup_tiles launch (6 values)
extern "C" int pv_debug_read_pstamps(pv_ctx* ctx, unsigned long long* out) {
    int64_t* d = nullptr;
    if (pv_get(ctx, "sum.diag", (size_t)pvsum::D_NDIAG + pvsum::D_SPARE, &d)) return PV_ERR_HIP;
    PV_HIP(hipDeviceSynchronize());
    PV_HIP(hipMemcpy(out, d + pvsum::D_NDIAG, 6 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return PV_OK;
}
#endif
