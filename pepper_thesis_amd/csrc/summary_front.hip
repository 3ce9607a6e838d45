// summary_front.hip — the front end the image builders and the polisher's summary share: CIGAR scan, (read, tile) pair
// lists, the start-of-call kernels, and the workspace slots they fill. The kernels are launched from here only (the
// library is built without relocatable device code); the pipelines call the host functions of summary_launch.hpp.
#include "summary_launch.hpp"
#include "summary_scan.hpp"

namespace pvsum {
namespace {

// ---- K1 -------------------------------------------------------------------------------------------
// One wave per read. CIGAR semantics of populate_summary_matrix (:353-565): M/=/X consume both,
// I and S consume the read, D consumes the reference, N and P consume BOTH (the REF_SKIP/PAD cases
// fall through into SOFT_CLIP, :556-561), H/B/unknown consume nothing. The walk stops at the first
// op that starts beyond ref_end (:355); those ops are marked inactive.
__global__ __launch_bounds__(256) void k_cigar_scan(SumArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= a.n_reads) return;
    const int g = wave_count_le(a.in.read_off, a.in.n_regions + 1, r, lane) - 1;
    if (lane == 0) a.read_region[r] = g;
    const int64_t c0 = a.in.cigar_off[r], c1 = a.in.cigar_off[r + 1];
    const bool skip = a.in.read_mapq[r] == 0;  // :619
    const int64_t R = a.in.ref_end[g] - a.in.ref_start[g] + 1;
    if (!skip && !a.polish && a.in.base_off[r + 1] - a.in.base_off[r] <= 0 && lane == 0) set_status(a.diag, PV_ERR_INVALID);
    int64_t ref_rel = a.in.read_pos[r] - a.in.ref_start[g];
    int64_t rd = 0;
    // Two trips of 64 ops per loop pass, each with its own CIGAR-word register that is reloaded (for two trips on) right
    // after its trip has used it: the words are requested about one and a half trips ahead and no copy between registers
    // makes the wave wait for a load it has just issued (a rotating pair did: s_waitcnt vmcnt(0) at every loop end).
    auto trip = [&](const uint32_t w, const int64_t cb) {
        const int64_t c = cb + lane;
        const int op = w & 0xF;
        const int64_t len = c < c1 ? (int64_t)(w >> 4) : 0;
        const bool cr = (op == 0 || op == 7 || op == 8 || op == 2 || op == 3 || op == 6);
        // P2: REF_SKIP and PAD share the DEL case (summary_generator.cpp:100-114) and consume the reference only
        const bool cq = (op == 0 || op == 7 || op == 8 || op == 1 || op == 4 || (!a.polish && (op == 3 || op == 6)));
        const int64_t dr = cr ? len : 0, dq = cq ? len : 0;
        // 64 lengths below 2^25 sum to less than 2^31: the 32-bit DPP scan is exact for every real CIGAR; anything longer takes
        // the 64-bit shuffle scan
        int64_t ir, iq;
        if (__ballot(len >= (1ll << 25)) == 0) {
            ir = wave_incl_scan32((int)dr, lane);
            iq = wave_incl_scan32((int)dq, lane);
        } else {
            ir = wave_incl_scan(dr, lane);
            iq = wave_incl_scan(dq, lane);
        }
        const int64_t my_ref = ref_rel + ir - dr, my_rd = rd + iq - dq;
        if (c < c1) {
            const bool active = !skip && my_ref < R;
            if (active && (my_ref < -(1ll << 30) || my_rd > (1ll << 30))) set_status(a.diag, PV_ERR_LIMIT);
            a.op_ref[c] = active ? (int32_t)my_ref : OP_INACTIVE;
            a.op_rd[c] = (int32_t)my_rd;
            if (a.polish) a.op_read[c] = (int32_t)r;   // only k_polish_insert walks op -> read
            if (a.polish) a.op_flag[c] = 0;   // (the image builders no longer keep a per-op flag: k_collect repeats the test)
        }
        ref_rel += last_lane(ir);
        rd += last_lane(iq);
    };
    auto fetch = [&](int64_t cb) -> uint32_t { return cb + lane < c1 ? a.in.cigar[cb + lane] : 0u; };
    uint32_t w_a = fetch(c0), w_b = fetch(c0 + 64);
    for (int64_t cb = c0; cb < c1; cb += 128) {
        trip(w_a, cb);
        w_a = fetch(cb + 128);
        if (cb + 64 >= c1) break;
        trip(w_b, cb + 64);
        w_b = fetch(cb + 192);
    }
    // Column span that this read can touch: every effect of populate_summary_matrix lies between the
    // column before its first position (an insert anchored at pos-1 after a leading soft clip) and its
    // last reference-consumed column, clipped to the region. One (read, tile) pair per overlapped tile.
    int64_t lo = a.in.read_pos[r] - a.in.ref_start[g] - 1, hi = ref_rel - 1;
    if (lo < 0) lo = 0;
    if (hi > R - 1) hi = R - 1;
    const int64_t cb0 = a.in.ref_off[g];
    int32_t t0 = 0, t1 = -1;
    if (!skip && hi >= lo) { t0 = (int32_t)((cb0 + lo) / TILE_COLS); t1 = (int32_t)((cb0 + hi) / TILE_COLS); }
    if (lane == 0) { a.read_t0[r] = t0; a.read_t1[r] = t1; }
    for (int32_t t = t0 + lane; t <= t1; t += 64) atomicAdd(&a.tile_cnt[t], 1);
}

// One wave per read: claim a slot in the pair list of every tile the read overlaps and record the op range [op_lo, op_hi)
// of the read that can touch the tile (an op starting one column past the tile may still anchor an indel on the tile's last
// column). The ranges come from ONE coalesced pass over the read's per-op start columns: an op whose start column and its
// predecessor's lie on different sides of a tile boundary is that boundary's lower / upper bound (start columns ascend), so
// each lane looks at its op and its left neighbour's and writes the boundaries between them to a per-wave LDS table. That was
// two binary searches per (read, tile) lane - ~20 dependent scattered probes - and 31 us per 16 regions; reads over more
// than TF_CAP tiles (regions beyond 130 kb) still search.
constexpr int TF_CAP = 256;
__global__ __launch_bounds__(256) void k_tile_fill(SumArgs a) {
    // per wave: lower bound of every 64-column boundary from the first column of tile t0 to that of tile t1 + 1, upper bound of
    // the tile boundaries
    // (16-bit op offsets from the read's first op: 18 KB per workgroup, so that eight of them still fit a CU; a read with more
    // than 65535 ops - or over more than TF_CAP tiles - takes the searches and leaves no sub-tile index)
    __shared__ uint16_t s_lo[4][TF_CAP * SUB_N + 2];
    __shared__ int32_t s_hi[4][TF_CAP + 1];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * 4 + wv;
    if (r >= a.n_reads || a.diag[D_STATUS] != 0) return;
    const int32_t t0 = a.read_t0[r], t1 = a.read_t1[r];
    if (t1 < t0) return;
    const int g = a.read_region[r];
    const int64_t cb0 = a.in.ref_off[g];
    const int32_t c0 = (int32_t)a.in.cigar_off[r], c1 = (int32_t)a.in.cigar_off[r + 1];
    const int nb = t1 - t0 + 2;   // boundaries: first columns of tiles t0 .. t1 + 1
    const bool table = nb <= TF_CAP + 1 && c1 - c0 <= 65535;
    if (table) {
        for (int i = lane; i < nb; i += 64) s_hi[wv][i] = c1;                         // no op behind the boundary
        for (int i = lane; i < (nb - 1) * SUB_N + 1; i += 64) s_lo[wv][i] = (uint16_t)(c1 - c0);   // no op at or behind the boundary
        auto fetch = [&](int32_t cb) -> int32_t { return cb + lane < c1 ? a.op_ref[cb + lane] : OP_INACTIVE; };
        int32_t carry = -0x7fffffff - 1;   // "start column" of the op before the first
        auto trip = [&](const int32_t x, const int32_t cb) {
            const int32_t c = cb + lane;
            int32_t p = __builtin_amdgcn_update_dpp(0, x, 0x138, 0xf, 0xf, false);   // wave_shr:1: the left neighbour's start column
            if (lane == 0) p = carry;
            if (c < c1 && p != x) {
                // boundaries b_t = t * TILE_COLS - cb0 (region-relative), t0 <= t <= t1 + 1
                const int64_t pp = (int64_t)p + cb0, xx = (int64_t)x + cb0;
                // lower bound of the 64-column boundaries u (column 64 u, counted from the first column of tile t0): p < b_u <= x
                const int64_t org = (int64_t)t0 * TILE_COLS;
                int64_t lo_a = ((pp - org) >> 6) + 1, lo_b = (xx - org) >> 6;
                int64_t hi_a = (pp + 511) >> 9, hi_b = ((xx + 511) >> 9) - 1;    // upper bound of the tile boundaries: p <= b_t < x
                static_assert(TILE_COLS == 512 && SUB_COLS == 64, ">> 9, >> 6");
                const int64_t u_last = (int64_t)(nb - 1) * SUB_N;
                if (lo_a < 0) lo_a = 0;
                if (hi_a < t0) hi_a = t0;
                if (lo_b > u_last) lo_b = u_last;
                if (hi_b > (int64_t)t1 + 1) hi_b = (int64_t)t1 + 1;
                for (int64_t u = lo_a; u <= lo_b; u++) s_lo[wv][u] = (uint16_t)(c - c0);
                for (int64_t t = hi_a; t <= hi_b; t++) s_hi[wv][t - t0] = c;
            }
            carry = __builtin_amdgcn_readlane(x, 63);
        };
        int32_t x_a = fetch(c0), x_b = fetch(c0 + 64);   // (two trips per pass, registers reloaded after use: see k_cigar_scan)
        for (int32_t cb = c0; cb < c1; cb += 128) {
            trip(x_a, cb);
            x_a = fetch(cb + 128);
            if (cb + 64 >= c1) break;
            trip(x_b, cb + 64);
            x_b = fetch(cb + 192);
        }
    }
    for (int32_t t = t0 + lane; t <= t1; t += 64) {
        int32_t op_lo, op_hi;
        PairRec pr;
        pr.subw[0] = pr.subw[1] = pr.subw[2] = pr.subw[3] = 0u;
        if (table) {
            const uint16_t* lo_t = &s_lo[wv][(t - t0) * SUB_N];
            const int32_t lower = c0 + lo_t[0];                     // first op with op_ref >= first column of tile t
            op_lo = lower > c0 ? lower - 1 : c0;
            op_hi = s_hi[wv][t + 1 - t0];                           // first op with op_ref > first column of tile t + 1
#pragma unroll
            for (int k = 0; k <= SUB_N; k++) {
                const int32_t d = c0 + (int32_t)lo_t[k] - op_lo;
                pr.subw[k >> 2] |= (uint32_t)(d > 255 ? 255 : d) << (8 * (k & 3));
            }
            pr.subw[(SUB_N + 1) >> 2] |= 1u << (8 * ((SUB_N + 1) & 3));
        } else {
            const int64_t tlo = (int64_t)t * TILE_COLS - cb0, thi = tlo + TILE_COLS - 1;  // region-relative columns
            int32_t lo = c0, hi = c1;  // first op with op_ref >= tlo
            while (lo < hi) { const int32_t mid = (lo + hi) >> 1; if ((int64_t)a.op_ref[mid] < tlo) lo = mid + 1; else hi = mid; }
            op_lo = lo > c0 ? lo - 1 : c0;
            lo = op_lo; hi = c1;  // first op with op_ref > thi + 1
            while (lo < hi) { const int32_t mid = (lo + hi) >> 1; if ((int64_t)a.op_ref[mid] <= thi + 1) lo = mid + 1; else hi = mid; }
            op_hi = lo;
        }
        const int32_t slot = a.tile_off[t] + atomicAdd(&a.tile_fill[t], 1);
        pr.read = (int32_t)r; pr.op_lo = op_lo; pr.op_hi = op_hi; pr.col_base = (int32_t)cb0;
        pr.R = (int32_t)(a.in.ref_end[g] - a.in.ref_start[g] + 1);
        pr.c_last = c1 - 1;
        pr.ref_len = (int32_t)(a.in.ref_off[g + 1] - cb0);
        pr.rev = a.in.read_flags[r] & 1;
        if (a.hp) {
            // region_summary_hp.cpp: REF-count planes and the allele maps take "hp_tag == 0 || hp_tag == k" (:395-402, :415-422);
            // the symbol planes take both sets for tag 0, set 1 for tag 1 and set 2 for ANY other tag (:454-462, get_feature_index :197)
            const int32_t tag = a.read_hp ? a.read_hp[r] : 0;
            const int cs = ((tag == 0 || tag == 1) ? 1 : 0) | ((tag == 0 || tag == 2) ? 2 : 0);
            const int ss = tag == 0 ? 3 : (tag == 1 ? 1 : 2);
            pr.rev |= (cs << 1) | (ss << 3);
        }
        pr.base0 = a.in.base_off[r];
        pr.seq_end = a.in.base_off[r + 1];
        a.pairs[slot] = pr;
    }
}

// tile pair counts -> offsets, total -> diag[D_NPAIRS]; over the pair workspace: nothing is filled or walked
__global__ __launch_bounds__(1024) void k_scan_tiles(SumArgs a) {
    __shared__ int64_t s_w[32];
    const int64_t total = block_excl_scan<int32_t>(a.tile_cnt, a.tile_off, a.n_tiles, s_w);
    if (total > a.max_pairs) {
        if (threadIdx.x == 0) set_status(a.diag, PV_ERR_LIMIT);
        for (int64_t t = threadIdx.x; t < a.n_tiles; t += 1024) a.tile_cnt[t] = 0;
    }
    if (threadIdx.x == 0) a.diag[D_NPAIRS] = total;
}

// single-block exclusive scan of n int32 values; total -> *total_out (int64) (polisher pipeline)
__global__ __launch_bounds__(1024) void k_scan_i32(const int32_t* in, int32_t* out, int64_t n_fixed,
                                                   const int64_t* n_ptr, int64_t n_cap, int64_t* total_out) {
    __shared__ int64_t s_w[32];
    int64_t n = n_ptr ? *n_ptr : n_fixed;
    if (n > n_cap) n = n_cap;
    const int64_t total = block_excl_scan<int32_t>(in, out, n, s_w);
    if (threadIdx.x == 0 && total_out) *total_out = total;
}

// start of a call: the diagnostics block and the per-tile pair counters / fill cursors (one launch instead of a kernel
// and two memsets)
__global__ __launch_bounds__(256) void k_init(SumArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < D_NDIAG + 8) a.diag[i] = 0;
    if (i < a.n_tiles) {
        a.tile_cnt[i] = 0;
        a.tile_fill[i] = 0;
        if (a.blk_cnt) {  // (builder pipelines; the polisher's has no site lists)
            a.blk_cnt[i] = 0;
            a.tile_g0[i] = thread_count_le(a.in.ref_off, a.in.n_regions + 1, i * TILE_COLS) - 1;
        }
    }
}

// a read reaches a column at most once, so a region's read count bounds every counter of its columns: the 16-bit planes are
// exact while it stays within MAX_REGION_READS. (Runs behind k_init, which zeroes the status words.)
__global__ __launch_bounds__(256) void k_check_depth(SumArgs a) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g < a.in.n_regions && a.in.read_off[g + 1] - a.in.read_off[g] > MAX_REGION_READS) {
        a.diag[D_DEPTH] = 1;
        set_status(a.diag, PV_ERR_LIMIT);
    }
}

}  // namespace

int front_claim(pv_ctx* ctx, SumArgs& a) {
    PV_CHECK(a.n_cols < (1ll << 31) - 2048 && a.n_cigar < (1ll << 31) && a.n_reads < (1ll << 31), PV_ERR_LIMIT,
             "batch too large for 32-bit column/op indices (cols %lld, ops %lld)", (long long)a.n_cols, (long long)a.n_cigar);
    a.n_tiles = (a.n_cols + TILE_COLS - 1) / TILE_COLS;
    const int64_t nc1 = a.n_cigar > 0 ? a.n_cigar : 1, nr1 = a.n_reads > 0 ? a.n_reads : 1;
    int rc;
    if ((rc = pv_get(ctx, "sum.op_ref", nc1, &a.op_ref))) return rc;
    if ((rc = pv_get(ctx, "sum.op_rd", nc1, &a.op_rd))) return rc;
    if ((rc = pv_get(ctx, "sum.op_flag", nc1, &a.op_flag))) return rc;
    if ((rc = pv_get(ctx, "sum.read_region", nr1, &a.read_region))) return rc;
    if ((rc = pv_get(ctx, "sum.read_t0", nr1, &a.read_t0))) return rc;
    if ((rc = pv_get(ctx, "sum.read_t1", nr1, &a.read_t1))) return rc;
    if ((rc = pv_get(ctx, "sum.tile_cnt", a.n_tiles, &a.tile_cnt))) return rc;
    if ((rc = pv_get(ctx, "sum.tile_off", a.n_tiles, &a.tile_off))) return rc;
    if ((rc = pv_get(ctx, "sum.tile_fill", a.n_tiles, &a.tile_fill))) return rc;
    // a read overlaps at most span/TILE_COLS + 2 tiles; the exact pair count is only known on the device, so the caller
    // bounds it (default_limits, polish_limits) and k_scan_tiles reports an overflow
    if ((rc = pv_get(ctx, "sum.pairs", a.max_pairs, &a.pairs))) return rc;
    if ((rc = pv_get(ctx, "sum.diag", (size_t)D_NDIAG + D_SPARE, &a.diag))) return rc;
    return PV_OK;
}

void front_init(const SumArgs& a, hipStream_t st) {
    k_init<<<grid_for(std::max<int64_t>(a.n_tiles, D_NDIAG + 8), 256), 256, 0, st>>>(a);
}

void front_check_depth(const SumArgs& a, hipStream_t st) {
    if (a.in.n_regions > 0) k_check_depth<<<grid_for(a.in.n_regions, 256), 256, 0, st>>>(a);
}

void front_pairs(pv_ctx* ctx, const SumArgs& a, hipStream_t st) {
    if (a.n_reads > 0) { pv_prof_scope ps(ctx, "k_cigar_scan", st); k_cigar_scan<<<grid_for(a.n_reads, 4), 256, 0, st>>>(a); }
    k_scan_tiles<<<1, 1024, 0, st>>>(a);
    if (a.n_reads > 0) { pv_prof_scope ps(ctx, "k_tile_fill", st); k_tile_fill<<<grid_for(a.n_reads, 4), 256, 0, st>>>(a); }
}

void front_scan_i32(const int32_t* in, int32_t* out, int64_t n, int64_t* total_out, hipStream_t st) {
    k_scan_i32<<<1, 1024, 0, st>>>(in, out, n, nullptr, n, total_out);
}
}  // namespace pvsum
