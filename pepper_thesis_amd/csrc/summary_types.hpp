// summary_types.hpp — constants, records and small device helpers shared by the summary builders' translation units
// (summary_front.hip, summary_builder.hip, summary_polish.hip, summary_host.hip).
#pragma once
#include "pv_common.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace pvsum {

constexpr int NCNT = 21;   // counters of a column
typedef uint32_t cnt_u32x4 __attribute__((ext_vector_type(4)));
constexpr int CNT_STRIDE = 24, CNT_STRIDE_HP = 40;   // counters of a column, padded to whole 16-byte granules (48 / 80 bytes)
static_assert(NCNT <= CNT_STRIDE, "the 21 counters of the 26-plane form fit its stride");
typedef int16_t cnt_t;               // element of the global counter planes (they were int32: half the flush and gather bytes)
constexpr int MAX_REGION_READS = 32767;
constexpr int C_COV = 0, C_SNP = 1, C_INS = 2, C_DEL = 3, C_RARE = 4, C_PLANE = 5;
// haplotag-aware builder (region_summary_hp.cpp): the same four site counters, then 4 groups (set 1 fwd, set 1 rev,
// set 2 fwd, set 2 rev) x {REF count, A, C, G, T, I, D, *} holding the FINAL signed plane values (window plane
// 4 + 11*group for the REF count, 8 + 11*group + k for the symbols)
constexpr int NCNT_HP = 36, HC_PLANE = 4;
static_assert(NCNT_HP <= CNT_STRIDE_HP, "the 36 counters of the haplotag form fit its stride");
constexpr int32_t OP_INACTIVE = 0x7fffffff;
constexpr int UMAX = 1024;  // distinct alleles per site held in LDS
constexpr int UM_SMALL = 96; // table of the k_site_alleles instantiation for sites with few events
constexpr int TILE_COLS = 512;  // columns per pileup tile (one workgroup accumulates a tile in LDS)

enum { D_SPARE = 8 };
enum { D_NSITES = 0, D_NEVENTS = 1, D_NOUT = 2, D_STRBYTES = 3, D_STATUS = 4, D_NPAIRS = 5, D_NINS = 6, D_NROWS = 7, D_NCHUNKS = 8, D_NBIG = 9, D_NDIAG = 10 };
enum { D_DEPTH = D_NDIAG + 7 };      // set (with status PV_ERR_LIMIT) when a region holds more reads than the 16-bit planes can count

struct Event {  // 16 B
    int64_t src;  // index into bases (kind 1) or ref (kind 2)
    int32_t len;
    uint8_t type;   // 1 SNP 2 INS 3 DEL
    uint8_t rev;
    uint8_t kind;   // 1 bases, 2 ref
    uint8_t flags;  // bit0: is an allele observation; bit1: plane correction (lower-case acgt counted in an ACGT plane);
                    // bits 2-3 (haplotag form): the haplotype sets whose per-strand allele counts the observation joins
};

struct AlleleRec {  // 32 B
    int64_t src;
    int32_t len;
    int32_t total;
    int32_t fwd;
    int32_t rev;
    uint8_t type;
    uint8_t kind;  // 0 immediate byte, 1 bases, 2 ref
    uint8_t imm;
    uint8_t pad;
    int32_t pad2;
};

constexpr int SUB_COLS = 64;                      // k_collect's sub-tile index: op offsets at every 64th column of the tile
constexpr int SUB_N = TILE_COLS / SUB_COLS;       // 8
struct PairRec {  // 64 B: everything a tile workgroup needs to walk one (read, tile) pair
    int32_t read, op_lo, op_hi, col_base;
    int32_t R, c_last, ref_len, rev;   // rev: bit0 strand; haplotag builder: bits 1-2 count sets, bits 3-4 symbol sets
    int64_t base0, seq_end;
    // byte k of subw, k = 0 .. SUB_N: (first op that starts at or behind column 64 k of the tile) - op_lo, saturated at 255; byte
    // SUB_N + 1: 1 when the index is there. A site at column c of the tile searches ops [op_lo + sub[c / 64], op_lo + sub[c / 64 + 1]]
    // only (~11 ops in one or two cache lines instead of ~90 in seven scattered probes).
    uint32_t subw[4];
    __device__ __forceinline__ int sub(int k) const {
        const uint32_t w = k < 4 ? subw[0] : (k < 8 ? subw[1] : subw[2]);
        return (int)((w >> (8 * (k & 3))) & 0xFFu);
    }
};
static_assert(sizeof(PairRec) == 64, "PairRec layout");

// What the per-site kernels need to know of a site before they can request anything else, as ONE 48-byte record written by
// k_site_rank: they are chains of dependent round trips at full occupancy (~3 us each under that load), and column -> region
// -> region geometry / tile range was two of those levels in each of them.
struct SiteHdr {
    int32_t col, col_base, R, g;      // global column, first column and length of its region, region
    int32_t p0, np, cov, flags;       // pair list of its tile, coverage, flags: bits 0-7 reference byte, bit 8: base observations wanted
                                      // (rare ones, or - haplotag form - SNP ones, were counted), bits 16-23: the site flag
    int64_t ref_start;                // of its region
    int32_t nev, pad;
};
static_assert(sizeof(SiteHdr) == 48, "SiteHdr layout");

struct SumArgs {
    pv_batch_in in;
    pv_params p;
    int64_t n_reads, n_bases, n_cigar, n_cols;
    int32_t* op_ref;
    int32_t* op_rd;
    int32_t* op_read;
    uint8_t* op_flag;
    int32_t* read_region;
    int32_t* read_t0;
    int32_t* read_t1;
    int32_t* tile_cnt;   // [n_tiles] (read, tile) pairs per tile
    int32_t* tile_off;   // [n_tiles] exclusive scan
    int32_t* tile_fill;
    PairRec* pairs;      // [n_pairs]
    int64_t n_tiles;
    int64_t max_pairs;
    int32_t qmin_snp;    // smallest integer quality q with (double)q >= min_snp_baseq (exact: q is an integer)
    cnt_t* cnt;
    uint8_t* flags;
    int32_t* blk_cnt;
    int32_t* site_col;
    int32_t* site_region;
    int32_t* site_nev;
    int32_t* site_evoff;
    int32_t* site_fill;
    int32_t* site_nemit;
    int64_t* site_strbytes;
    int32_t* site_outoff;
    int64_t* site_stroff;
    Event* ev;
    AlleleRec* rec;
    int64_t* diag;
    int64_t max_sites;
    int64_t max_events;
    pv_batch_out out;
    int64_t* d_counts;
    // ---- haplotag-aware builder only ----
    int32_t hp;               // 1: RegionalSummaryGeneratorHP semantics (48 planes, 21 rows)
    const int32_t* read_hp;   // [n_reads] type_read::hp_tag, or null (all 0)
    // ---- P2 (polisher) summary only ----
    int32_t polish;       // 1: CIGAR semantics of SummaryGenerator::iterate_over_read (N and P consume the reference only)
    int32_t seq_len, seq_step;  // chunk length, chunk length - overlap
    int32_t* pcnt;        // [PC_N][n_cols] plane-major: 10 features, coverage, longest insert
    int32_t* tile_g0;     // [n_tiles] region of each tile's first column
    SiteHdr* site_hdr;    // [max_sites]
    int32_t* big_sites;   // [max_sites] ranks of the sites whose events need the large allele table (diag[D_NBIG] of them)
    int32_t* ins_blk;     // [n_blk] insert rows per 1024-column block
    int32_t* ins_blkoff;  // [n_blk] exclusive scan
    int32_t* ins_off;     // [n_cols + 1] insert rows before every column
    int32_t* ins_cnt;     // [max_ins_rows][10]
    int64_t max_ins_rows;
    int64_t* reg_rows;    // [n_regions + 1] first flat row of every region
    int64_t* reg_chunks;  // [n_regions + 1] first chunk of every region
    uint8_t* flat_img;    // [flat_cap][10]
    int64_t* flat_pos;
    int32_t* flat_idx;
    uint16_t* flat_depth; // [flat_cap] or null: wanted only with pout.depth
    uint16_t* flat_counts; // [flat_cap][10] or null: wanted only with pout.counts
    int64_t flat_cap;
    pv_polish_out pout;
};

__device__ __forceinline__ int up(int c) { return (c >= 'a' && c <= 'z') ? c - 32 : c; }
__device__ __forceinline__ bool is_acgt(int c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }
// offset of get_feature_index's result from its strand start (region_summary.cpp:208-215): A1 C2 G3 T4 I5 D6 other 7
__device__ __forceinline__ int sym_of(int c) {
    c = up(c);
    return c == 'A' ? 1 : c == 'C' ? 2 : c == 'G' ? 3 : c == 'T' ? 4 : c == 'I' ? 5 : c == 'D' ? 6 : 7;
}
__device__ __forceinline__ int refcode(int c) {  // get_reference_feature_value, :165-172
    c = up(c);
    return c == 'A' ? 1 : c == 'C' ? 2 : c == 'G' ? 3 : c == 'T' ? 4 : 5;
}
__device__ __forceinline__ void set_status(int64_t* diag, int code) {
    atomicCAS((unsigned long long*)&diag[D_STATUS], 0ull, (unsigned long long)(long long)code);
}
__device__ __forceinline__ int upper_bound_i64(const int64_t* a, int n, int64_t v) {  // first idx with a[idx] > v
    int lo = 0, hi = n;
    while (lo < hi) {
        int mid = (lo + hi) >> 1;
        if (a[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// The same answer (number of entries <= v) for the short ascending offset tables of a batch (regions + 1 entries) in ONE round
// trip: every entry is requested at once and compared, instead of five dependent probes. wave_: v uniform over the wave, an
// entry per lane; thread_: independent loads in a short loop. Longer tables take the search.
__device__ __forceinline__ int wave_count_le(const int64_t* a, int n, int64_t v, int lane) {
    if (n > 64) return upper_bound_i64(a, n, v);
    const bool le = lane < n && a[lane] <= v;
    return __popcll(__ballot(le));
}
__device__ __forceinline__ int thread_count_le(const int64_t* a, int n, int64_t v) {
    if (n > 32) return upper_bound_i64(a, n, v);
    int c = 0;
    for (int i = 0; i < n; i++) c += a[i] <= v ? 1 : 0;
    return c;
}

__device__ __forceinline__ int64_t last_lane(int64_t v) {   // lane 63's value in every lane (scalar reads, no LDS permute)
    const unsigned lo = __builtin_amdgcn_readlane((unsigned)v, 63), hi = __builtin_amdgcn_readlane((unsigned)((uint64_t)v >> 32), 63);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
// inclusive wave prefix sums on the DPP path: four row shifts inside the 16-lane rows, then the row totals (row_bcast:15 into
// rows 1 and 3, row_bcast:31 into rows 2 and 3) - six DPP adds instead of six ds_bpermute round trips (twelve for the
// 64-bit form, whose halves move separately and are added as one number)
template <int CTRL, int ROWS>
__device__ __forceinline__ int64_t dpp_move64(int64_t x) {
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)x, CTRL, ROWS, 0xf, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)((uint64_t)x >> 32), CTRL, ROWS, 0xf, false);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ int64_t wave_incl_scan(int64_t v, int) {
    int64_t x = v;
    x += dpp_move64<0x111, 0xf>(x);   // row_shr:1
    x += dpp_move64<0x112, 0xf>(x);   // row_shr:2
    x += dpp_move64<0x114, 0xf>(x);   // row_shr:4
    x += dpp_move64<0x118, 0xf>(x);   // row_shr:8
    x += dpp_move64<0x142, 0xa>(x);   // row_bcast:15
    x += dpp_move64<0x143, 0xc>(x);   // row_bcast:31
    return x;
}
__device__ __forceinline__ int wave_incl_scan32(int v, int) {
    int x = v;
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, false);   // row_shr:1
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, false);   // row_shr:2
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, false);   // row_shr:4
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, false);   // row_shr:8
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);   // row_bcast:15
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);   // row_bcast:31
    return x;
}

// ---- tile kernels (k_pileup_tiles, k_polish_tiles) ---------------------------------------------------
constexpr int PT_THREADS = 512;
constexpr int PT_PB = 128;  // pairs per batch
constexpr int PT_GPL = 1;   // groups of 4 consecutive bases per thread per trip (groups strided by the block size)
// counters of a tile live in LDS with the column index swizzled so that the 64 lanes of a wave, which hold columns
// c, c+4, c+8, ... for the same group element, hit 64 consecutive banks
// (= ((lc & 3) << 7) | (lc >> 2) for 0 <= lc < 512, as one multiply-add and one bit-field extract: lc * 513 = lc | lc << 9)
#define SW(lc) ((int)((((unsigned)(lc) * 513u) >> 2) & 511u))
static_assert(TILE_COLS == 512, "SW() assumes 512-column tiles");

// (s_wsum: two sets of wave totals used in turn - `turn` counts the calls - so that one barrier per call is enough: a set is
// written again two calls later, and every thread has passed the barrier of the call in between only after all of them have
// read this one)
__device__ __forceinline__ int block_incl_scan512(int v, int* s_wsum, int tid, int& turn) {
    const int lane = tid & 63, wv = tid >> 6;
    int* ws = s_wsum + (turn & 1) * (PT_THREADS / 64);
    turn++;
    const int inc = wave_incl_scan32(v, lane);
    if (lane == 63) ws[wv] = inc;
    __syncthreads();
    int off = 0;
#pragma unroll
    for (int k = 0; k < PT_THREADS / 64; k++) off += (k < wv) ? ws[k] : 0;
    return inc + off;
}

static inline unsigned int grid_for(int64_t n, int per) { return (unsigned int)((n + per - 1) / per); }

}  // namespace pvsum
