// batch_select.hip — selection of a flat batch (pv_batch_in) by haplotype: `polish -hp` runs its chain once per haplotype on
// the reads of that haplotype, and the builder and the realigner take contiguous offset arrays only.
//
// Rule (include/pepper_hip.h): read r is kept iff read_hp == NULL, read_hp[r] == 0 or read_hp[r] == haplotype; the output is
// the input without the dropped reads, offsets rebuilt from 0, region arrays shared with the input.
//
// Kernels (asynchronous on one stream, no host read-back, no global atomics):
//   k_sel_totals   one workgroup per 4096 reads (a thread owns 8): keep flag, kept bases and kept cigar words of the chunk
//                  summed to one record per chunk; the offset checks (base_off / cigar_off / read_off monotone, the closing
//                  entries against n_bases / n_cigar / n_reads) run here, before any payload byte is read.
//   k_sel_scan     the same grid: a chunk adds up the records in front of it (its carry) and all of them (totals, status),
//                  scans its own three columns side by side and scatters the per-read records and the new offsets to the
//                  reads' new indices. new_idx [n_reads + 1] stays in the workspace for the regions; the first workgroup
//                  writes the closing entries and d_counts.
//   k_sel_regions  read_off[g] = new_idx[read_off_in[g]].
//   k_sel_gather   the payload, split by 16 KB pieces of the OUTPUT (a 50-base read and a 100 kb read cost what they weigh): a
//                  lane owns four 16-byte-aligned 16-byte groups of the destination, finds a group's read by a search in the new
//                  offsets (narrowed to the piece's reads by two waves first, 64 probes a step) and, where the group lies in one read, loads its
//                  16 source bytes with one load of alignment 1 (global_load_dwordx4 on gfx950: the source is shifted against
//                  the destination by any number of bytes) and stores them with one global_store_dwordx4. Groups that cross a
//                  read's end, and the partial groups at both ends of the array, go element by element. blockIdx.y picks
//                  bases or quals (same offsets); the cigar is the same kernel on 4-byte words.
#include "pv_common.hpp"

namespace {

constexpr int SEL_V = 8;                       // reads per thread
constexpr int SEL_THREADS = 512;                 // 256 VGPRs a thread: the scan holds 8 reads' offsets and records at once
constexpr int64_t SEL_CHUNK = (int64_t)SEL_V * SEL_THREADS;
constexpr int SEL_G_THREADS = 256;             // gather: 256 lanes x 16 bytes x 4 groups = one 16 KB piece
constexpr int SEL_G_GROUPS = 4;

struct SelArgs {
    int n_regions;
    int haplotype;
    int64_t n_reads, n_bases, n_cigar;
    const int64_t* read_off;
    const int64_t* read_pos;
    const uint8_t* read_flags;
    const uint8_t* read_mapq;
    const int64_t* base_off;
    const int64_t* cigar_off;
    const int32_t* read_hp;
    int64_t cap_reads, cap_bases, cap_cigar;
    int64_t* o_read_off;
    int64_t* o_read_pos;
    uint8_t* o_read_flags;
    uint8_t* o_read_mapq;
    int64_t* o_base_off;
    int64_t* o_cigar_off;
    int32_t* o_read_hp;      // optional
    int64_t* o_src_read;     // optional: the caller's copy of src
    int64_t* src;            // [n_reads] workspace: input index of every kept read
    int64_t* new_idx;        // [n_reads + 1] workspace
    int64_t* chunk_tot;      // [chunks][4] workspace: reads, bases, words kept, fault
    int64_t n_chunks;
    int64_t* counts;
};

__device__ __forceinline__ int64_t wave_sum(int64_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
// sum of v over the workgroup, the same in every thread; s: 16 cells, reusable after the call
__device__ __forceinline__ int64_t block_sum(int64_t v, int64_t* s) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    int64_t t = 0;
#pragma unroll
    for (int k = 0; k < SEL_THREADS / 64; k++) t += s[k];
    __syncthreads();
    return t;
}
__device__ __forceinline__ int64_t wave_incl(int64_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t y = __shfl_up(v, d, 64);
        if (lane >= d) v += y;
    }
    return v;
}

__device__ __forceinline__ bool sel_keep(const SelArgs& a, int64_t r) {
    if (!a.read_hp) return true;
    const int32_t t = a.read_hp[r];
    return t == 0 || t == a.haplotype;
}

// a thread's 8 reads: keep flags and offsets (a decreasing offset counts as length 0 and as a fault). The lengths are
// worked out where they are used: held for all 8 reads as well they only cost registers.
struct SelOwn {
    unsigned keep;   // bit e: read r0 + e is kept
    int fault;
    int64_t b[SEL_V + 1], c[SEL_V + 1];
    __device__ __forceinline__ int kept(int e) const { return (int)((keep >> e) & 1u); }
    __device__ __forceinline__ int64_t nb(int e) const { return kept(e) && b[e + 1] > b[e] ? b[e + 1] - b[e] : 0; }
    __device__ __forceinline__ int64_t nc(int e) const { return kept(e) && c[e + 1] > c[e] ? c[e + 1] - c[e] : 0; }
};
__device__ __forceinline__ SelOwn sel_own(const SelArgs& a, int64_t r0) {
    SelOwn o;
    o.fault = 0;
    o.keep = 0;
#pragma unroll
    for (int e = 0; e <= SEL_V; e++) {
        const int64_t r = r0 + e <= a.n_reads ? r0 + e : a.n_reads;
        o.b[e] = a.base_off[r];
        o.c[e] = a.cigar_off[r];
    }
#pragma unroll
    for (int e = 0; e < SEL_V; e++) {
        const bool in = r0 + e < a.n_reads;
        if (in && (o.b[e + 1] < o.b[e] || o.c[e + 1] < o.c[e])) o.fault = 1;
        if (in && sel_keep(a, r0 + e)) o.keep |= 1u << e;
    }
    return o;
}

__global__ __launch_bounds__(SEL_THREADS) void k_sel_totals(SelArgs a) {
    __shared__ int64_t s[SEL_THREADS / 64];
    const int64_t r0 = (int64_t)blockIdx.x * SEL_CHUNK + (int64_t)threadIdx.x * SEL_V;
    int64_t nr = 0, nb = 0, nc = 0, fault = 0;
    if (r0 < a.n_reads) {
        const SelOwn o = sel_own(a, r0);
#pragma unroll
        for (int e = 0; e < SEL_V; e++) { nr += o.kept(e); nb += o.nb(e); nc += o.nc(e); }
        fault = o.fault;
    }
    // the regions, spread over the grid
    const int64_t gs = (int64_t)gridDim.x * SEL_THREADS;
    for (int64_t g = (int64_t)blockIdx.x * SEL_THREADS + threadIdx.x; g < a.n_regions; g += gs)
        if (a.read_off[g + 1] < a.read_off[g]) fault = 1;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (a.read_off[0] != 0 || a.read_off[a.n_regions] != a.n_reads) fault = 1;
        if (a.base_off[0] < 0 || a.cigar_off[0] < 0) fault = 1;
        if (a.base_off[a.n_reads] > a.n_bases || a.cigar_off[a.n_reads] > a.n_cigar) fault = 1;
    }
    nr = block_sum(nr, s);
    nb = block_sum(nb, s);
    nc = block_sum(nc, s);
    fault = block_sum(fault, s);
    if (threadIdx.x == 0) {
        int64_t* t = a.chunk_tot + (int64_t)blockIdx.x * 4;
        t[0] = nr; t[1] = nb; t[2] = nc; t[3] = fault;
    }
}

__device__ __forceinline__ int64_t sel_status(const SelArgs& a, int64_t nr, int64_t nb, int64_t nc, int64_t fault) {
    if (fault) return PV_ERR_INVALID;
    return nr > a.cap_reads || nb > a.cap_bases || nc > a.cap_cigar ? PV_ERR_CAPACITY : PV_OK;
}

__global__ __launch_bounds__(SEL_THREADS) void k_sel_scan(SelArgs a) {
    __shared__ int64_t s[SEL_THREADS / 64];
    __shared__ int64_t s_w[3][SEL_THREADS / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    // carry of this chunk and the totals of the batch
    int64_t c_r = 0, c_b = 0, c_c = 0, t_r = 0, t_b = 0, t_c = 0, fault = 0;
    for (int64_t k = threadIdx.x; k < a.n_chunks; k += SEL_THREADS) {
        const int64_t* t = a.chunk_tot + k * 4;
        const int64_t x0 = t[0], x1 = t[1], x2 = t[2];
        t_r += x0; t_b += x1; t_c += x2; fault += t[3];
        if (k < (int64_t)blockIdx.x) { c_r += x0; c_b += x1; c_c += x2; }
    }
    c_r = block_sum(c_r, s); c_b = block_sum(c_b, s); c_c = block_sum(c_c, s);
    t_r = block_sum(t_r, s); t_b = block_sum(t_b, s); t_c = block_sum(t_c, s);
    fault = block_sum(fault, s);
    const int64_t status = sel_status(a, t_r, t_b, t_c, fault);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const bool bad = status == PV_ERR_INVALID;
        a.counts[0] = bad ? 0 : t_r; a.counts[1] = bad ? 0 : t_b; a.counts[2] = bad ? 0 : t_c; a.counts[3] = status;
        if (!bad) {
            a.new_idx[a.n_reads] = t_r;
            if (t_r <= a.cap_reads) { a.o_base_off[t_r] = t_b; a.o_cigar_off[t_r] = t_c; }
        }
    }
    if (status == PV_ERR_INVALID) return;
    const int64_t r0 = (int64_t)blockIdx.x * SEL_CHUNK + (int64_t)threadIdx.x * SEL_V;
    SelOwn o;
    if (r0 < a.n_reads) {
        o = sel_own(a, r0);
    } else {
        o.keep = 0;
#pragma unroll
        for (int e = 0; e <= SEL_V; e++) { o.b[e] = 0; o.c[e] = 0; }
    }
    int64_t m_r = 0, m_b = 0, m_c = 0;
#pragma unroll
    for (int e = 0; e < SEL_V; e++) { m_r += o.kept(e); m_b += o.nb(e); m_c += o.nc(e); }
    const int64_t i_r = wave_incl(m_r, lane), i_b = wave_incl(m_b, lane), i_c = wave_incl(m_c, lane);
    if (lane == 63) { s_w[0][wv] = i_r; s_w[1][wv] = i_b; s_w[2][wv] = i_c; }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SEL_THREADS / 64; k++) {
        c_r += k < wv ? s_w[0][k] : 0;
        c_b += k < wv ? s_w[1][k] : 0;
        c_c += k < wv ? s_w[2][k] : 0;
    }
    int64_t j = c_r + i_r - m_r, ob = c_b + i_b - m_b, oc = c_c + i_c - m_c;
#pragma unroll
    for (int e = 0; e < SEL_V; e++) {
        const int64_t r = r0 + e;
        if (r < a.n_reads) {
            a.new_idx[r] = j;
            if (o.kept(e) && j < a.cap_reads) {
                a.src[j] = r;
                if (a.o_src_read) a.o_src_read[j] = r;
                a.o_read_pos[j] = a.read_pos[r];
                a.o_read_flags[j] = a.read_flags[r];
                a.o_read_mapq[j] = a.read_mapq[r];
                if (a.o_read_hp) a.o_read_hp[j] = a.read_hp ? a.read_hp[r] : 0;
                a.o_base_off[j] = ob;
                a.o_cigar_off[j] = oc;
            }
        }
        j += o.kept(e); ob += o.nb(e); oc += o.nc(e);
    }
}

__global__ void k_sel_regions(SelArgs a) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g > a.n_regions || a.counts[3] == PV_ERR_INVALID) return;
    a.o_read_off[g] = a.new_idx[a.read_off[g]];   // read_off was checked: 0 .. n_reads
}

// ---- payload ----------------------------------------------------------------------------------------------------------
typedef unsigned sel_u32x4 __attribute__((ext_vector_type(4)));

// last read j in [lo, hi] with off[j] <= o (off[lo] <= o is given)
__device__ __forceinline__ int64_t sel_find(const int64_t* off, int64_t lo, int64_t hi, int64_t o) {
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= o) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// the same by a whole wave (o, lo, hi wave-uniform): 64 probes a step, so three dependent loads find a read among 262 k where
// the binary search takes 18
__device__ __forceinline__ int64_t sel_find_wave(const int64_t* off, int64_t lo, int64_t hi, int64_t o, int lane) {
    while (lo < hi) {
        const int64_t step = (hi - lo) / 64 + 1;              // 64 * step > hi - lo: the probes reach hi
        const int64_t p = lo + (int64_t)(lane + 1) * step;
        const bool le = p <= hi && off[p] <= o;               // off is non-decreasing: true for the lanes below some c
        const int c = __popcll(__ballot(le));
        const int64_t top = lo + (int64_t)(c + 1) * step - 1;
        lo += (int64_t)c * step;
        hi = top < hi ? top : hi;
    }
    return lo;
}

struct GatherArgs {
    const int64_t* in_off;    // input offsets [n_reads + 1]
    const int64_t* out_off;   // new offsets [kept + 1]
    const int64_t* src;       // input index of a kept read
    const int64_t* counts;
    int which;                // index into counts of this payload's total (1 bases, 2 cigar)
    const void* in0; void* out0;   // blockIdx.y == 0
    const void* in1; void* out1;   // blockIdx.y == 1
};

// one 16-byte group of the destination: elements [o0, o0 + PER) of the output, clipped to [0, total); its read lies in [jlo, jhi]
template <typename T>
__device__ __forceinline__ void sel_group(const GatherArgs& g, const T* in, T* out, int64_t o0, int64_t total, int64_t jlo, int64_t jhi) {
    constexpr int PER = 16 / (int)sizeof(T);
    int64_t o1 = o0 + PER;
    const bool whole = o0 >= 0 && o1 <= total;
    if (o0 < 0) o0 = 0;
    if (o1 > total) o1 = total;
    if (o0 >= o1) return;
    int64_t j = sel_find(g.out_off, jlo, jhi, o0);
    int64_t end = g.out_off[j + 1];
    int64_t sp = g.in_off[g.src[j]] + (o0 - g.out_off[j]);
    if (whole && o1 <= end) {
        sel_u32x4 v;
        __builtin_memcpy(&v, in + sp, 16);   // alignment of T only
        *reinterpret_cast<sel_u32x4*>(out + o0) = v;
        return;
    }
    T e[PER];
#pragma unroll
    for (int k = 0; k < PER; k++) {
        const int64_t o = o0 + k;
        e[k] = 0;
        if (o < o1) {
            while (o >= end) {   // ends of empty reads are passed too; o < total = out_off[kept] ends the walk
                j++;
                end = g.out_off[j + 1];
                sp = g.in_off[g.src[j]];
            }
            e[k] = in[sp++];
        }
    }
    if (whole) {
        sel_u32x4 v;
        if constexpr (sizeof(T) == 4) {
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = (unsigned)e[k];
        } else {
#pragma unroll
            for (int q = 0; q < 4; q++)
                v[q] = (unsigned)e[4 * q] | ((unsigned)e[4 * q + 1] << 8) | ((unsigned)e[4 * q + 2] << 16) | ((unsigned)e[4 * q + 3] << 24);
        }
        *reinterpret_cast<sel_u32x4*>(out + o0) = v;
    } else {
#pragma unroll
        for (int k = 0; k < PER; k++) if (o0 + k < o1) out[o0 + k] = e[k];
    }
}

template <typename T>
__global__ __launch_bounds__(SEL_G_THREADS) void k_sel_gather(GatherArgs g) {
    constexpr int PER = 16 / (int)sizeof(T);            // elements per 16-byte group
    constexpr int64_t PIECE = (int64_t)PER * SEL_G_THREADS * SEL_G_GROUPS;
    __shared__ int64_t s_j[2];
    if (g.counts[3] != PV_OK) return;
    const int64_t total = g.counts[g.which], kept = g.counts[0];
    const T* in = (const T*)(blockIdx.y ? g.in1 : g.in0);
    T* out = (T*)(blockIdx.y ? g.out1 : g.out0);
    // groups are cut at the destination's 16-byte boundaries: group k covers elements [k * PER - d0, (k + 1) * PER - d0)
    const int64_t d0 = (int64_t)(((uintptr_t)out & 15) / sizeof(T));
    const int64_t p0 = (int64_t)blockIdx.x * PIECE - d0;
    if (p0 >= total) return;
    if (threadIdx.x < 128) {   // the reads of the piece's first and last element: a wave each
        const int w = threadIdx.x >> 6;
        const int64_t o = w == 0 ? (p0 > 0 ? p0 : 0) : (p0 + PIECE - 1 < total ? p0 + PIECE - 1 : total - 1);
        const int64_t j = sel_find_wave(g.out_off, 0, kept - 1, o, threadIdx.x & 63);   // total > 0, so kept > 0
        if ((threadIdx.x & 63) == 0) s_j[w] = j;
    }
    __syncthreads();
    const int64_t jlo = s_j[0], jhi = s_j[1];
#pragma unroll
    for (int u = 0; u < SEL_G_GROUPS; u++)
        sel_group<T>(g, in, out, p0 + ((int64_t)u * SEL_G_THREADS + threadIdx.x) * PER, total, jlo, jhi);
}

template <typename T>
static void sel_launch_gather(pv_ctx* ctx, const char* name, const GatherArgs& g, int64_t bound, int n_arrays, hipStream_t st) {
    constexpr int64_t PIECE = (int64_t)(16 / sizeof(T)) * SEL_G_THREADS * SEL_G_GROUPS;
    if (bound <= 0 || n_arrays <= 0) return;
    const int64_t pieces = (bound + PIECE - 1) / PIECE + 1;   // + 1: a destination that is not 16-byte aligned shifts the cut
    pv_prof_scope ps(ctx, name, st);
    k_sel_gather<T><<<dim3((unsigned)pieces, (unsigned)n_arrays), SEL_G_THREADS, 0, st>>>(g);
}

}  // namespace

extern "C" int pv_batch_select_hp_dev(pv_ctx* ctx, const pv_batch_in* in, const int32_t* read_hp, int64_t n_reads, int64_t n_bases,
                                      int64_t n_cigar, int haplotype, pv_select_out* out, int64_t* d_counts, void* stream) {
    PV_CHECK(ctx && in && out && d_counts, PV_ERR_INVALID, "null argument");
    PV_CHECK(haplotype >= 1, PV_ERR_INVALID, "select: haplotype must be 1 or above, got %d", haplotype);
    PV_CHECK(in->n_regions >= 0 && n_reads >= 0 && n_bases >= 0 && n_cigar >= 0 && out->read_capacity >= 0 &&
                 out->base_capacity >= 0 && out->cigar_capacity >= 0, PV_ERR_INVALID, "negative sizes");
    PV_CHECK(in->read_off && in->base_off && in->cigar_off && out->read_off && out->base_off && out->cigar_off, PV_ERR_INVALID,
             "select: offset arrays missing");
    PV_CHECK(n_reads == 0 || (in->read_pos && in->read_flags && in->read_mapq), PV_ERR_INVALID, "select: per-read arrays missing");
    PV_CHECK(out->read_capacity == 0 || (out->read_pos && out->read_flags && out->read_mapq), PV_ERR_INVALID,
             "select: per-read output arrays missing");
    PV_CHECK(n_bases == 0 || in->bases, PV_ERR_INVALID, "select: bases missing");
    PV_CHECK(n_cigar == 0 || in->cigar, PV_ERR_INVALID, "select: cigar missing");
    PV_CHECK(out->base_capacity == 0 || (out->bases && (out->quals || !in->quals)), PV_ERR_INVALID, "select: bases / quals output missing");
    PV_CHECK(out->cigar_capacity == 0 || out->cigar, PV_ERR_INVALID, "select: cigar output missing");
    PV_CHECK(((uintptr_t)out->cigar & 3) == 0 && ((uintptr_t)in->cigar & 3) == 0, PV_ERR_INVALID, "select: cigar arrays must be 4-byte aligned");
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = pv_pick_stream(ctx, stream);
    SelArgs a;
    memset(&a, 0, sizeof(a));
    a.n_regions = in->n_regions; a.haplotype = haplotype;
    a.n_reads = n_reads; a.n_bases = n_bases; a.n_cigar = n_cigar;
    a.read_off = in->read_off; a.read_pos = in->read_pos; a.read_flags = in->read_flags; a.read_mapq = in->read_mapq;
    a.base_off = in->base_off; a.cigar_off = in->cigar_off; a.read_hp = read_hp;
    a.cap_reads = out->read_capacity; a.cap_bases = out->base_capacity; a.cap_cigar = out->cigar_capacity;
    a.o_read_off = out->read_off; a.o_read_pos = out->read_pos; a.o_read_flags = out->read_flags; a.o_read_mapq = out->read_mapq;
    a.o_base_off = out->base_off; a.o_cigar_off = out->cigar_off; a.o_read_hp = out->read_hp; a.o_src_read = out->src_read;
    a.counts = d_counts;
    a.n_chunks = std::max<int64_t>(1, (n_reads + SEL_CHUNK - 1) / SEL_CHUNK);
    int rc;
    if ((rc = pv_get(ctx, "sel.src", (size_t)n_reads + 1, &a.src))) return rc;
    if ((rc = pv_get(ctx, "sel.new_idx", (size_t)n_reads + 1, &a.new_idx))) return rc;
    if ((rc = pv_get(ctx, "sel.chunk_tot", (size_t)a.n_chunks * 4, &a.chunk_tot))) return rc;
    pv_prof_scope ps_all(ctx, "polish_select", st);
    { pv_prof_scope ps(ctx, "k_sel_totals", st); k_sel_totals<<<(unsigned)a.n_chunks, SEL_THREADS, 0, st>>>(a); }
    { pv_prof_scope ps(ctx, "k_sel_scan", st); k_sel_scan<<<(unsigned)a.n_chunks, SEL_THREADS, 0, st>>>(a); }
    k_sel_regions<<<(unsigned)(in->n_regions / 256 + 1), 256, 0, st>>>(a);
    GatherArgs g;
    memset(&g, 0, sizeof(g));
    g.src = a.src; g.counts = d_counts;
    g.in_off = in->base_off; g.out_off = out->base_off; g.which = 1;
    g.in0 = in->bases; g.out0 = out->bases; g.in1 = in->quals; g.out1 = out->quals;
    sel_launch_gather<uint8_t>(ctx, "k_sel_gather_bases", g, std::min(n_bases, out->base_capacity), in->quals ? 2 : 1, st);
    g.in_off = in->cigar_off; g.out_off = out->cigar_off; g.which = 2;
    g.in0 = in->cigar; g.out0 = out->cigar; g.in1 = nullptr; g.out1 = nullptr;
    sel_launch_gather<uint32_t>(ctx, "k_sel_gather_cigar", g, std::min(n_cigar, out->cigar_capacity), 1, st);
    PV_HIP(hipGetLastError());
    return PV_OK;
}

template <typename T>
static int sel_stage(pv_ctx* ctx, const char* name, const T* src, size_t n, const T** dst, hipStream_t st) {
    T* d = nullptr;
    int rc = pv_get(ctx, name, n > 0 ? n : 1, &d);
    if (rc) return rc;
    if (n > 0 && src) PV_HIP(hipMemcpyAsync(d, src, n * sizeof(T), hipMemcpyHostToDevice, st));
    *dst = d;
    return PV_OK;
}
template <typename T>
static int sel_fetch(T* dst, const T* src, int64_t n, hipStream_t st) {
    if (n > 0 && dst) PV_HIP(hipMemcpyAsync(dst, src, (size_t)n * sizeof(T), hipMemcpyDeviceToHost, st));
    return PV_OK;
}

extern "C" int pv_batch_select_hp(pv_ctx* ctx, const pv_batch_in* in, const int32_t* read_hp, int haplotype, pv_select_out* out) {
    PV_CHECK(ctx && in && out, PV_ERR_INVALID, "null argument");
    PV_CHECK(haplotype >= 1, PV_ERR_INVALID, "select: haplotype must be 1 or above, got %d", haplotype);
    const int G = in->n_regions;
    PV_CHECK(G >= 0 && out->read_capacity >= 0 && out->base_capacity >= 0 && out->cigar_capacity >= 0, PV_ERR_INVALID, "negative sizes");
    PV_CHECK(in->read_off && in->base_off && in->cigar_off && out->read_off && out->base_off && out->cigar_off, PV_ERR_INVALID,
             "select: offset arrays missing");
    // the offsets size the copies below, so the host form checks them before it reads through them
    PV_CHECK(in->read_off[0] == 0, PV_ERR_INVALID, "select: read_off[0] must be 0");
    for (int g = 0; g < G; g++)
        PV_CHECK(in->read_off[g + 1] >= in->read_off[g], PV_ERR_INVALID, "select: read_off decreases behind region %d", g);
    const int64_t n_reads = in->read_off[G];
    PV_CHECK(in->base_off[0] >= 0 && in->cigar_off[0] >= 0, PV_ERR_INVALID, "select: negative offsets");
    for (int64_t r = 0; r < n_reads; r++)
        PV_CHECK(in->base_off[r + 1] >= in->base_off[r] && in->cigar_off[r + 1] >= in->cigar_off[r], PV_ERR_INVALID,
                 "select: offsets of read %lld decrease", (long long)r);
    const int64_t n_bases = in->base_off[n_reads], n_cigar = in->cigar_off[n_reads];
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    pv_batch_in d = *in;
    const int32_t* d_hp = nullptr;
    int rc;
    if ((rc = sel_stage(ctx, "sels.read_off", in->read_off, (size_t)G + 1, &d.read_off, st))) return rc;
    if ((rc = sel_stage(ctx, "sels.read_pos", in->read_pos, (size_t)n_reads, &d.read_pos, st))) return rc;
    if ((rc = sel_stage(ctx, "sels.read_flags", in->read_flags, (size_t)n_reads, &d.read_flags, st))) return rc;
    if ((rc = sel_stage(ctx, "sels.read_mapq", in->read_mapq, (size_t)n_reads, &d.read_mapq, st))) return rc;
    if ((rc = sel_stage(ctx, "sels.base_off", in->base_off, (size_t)n_reads + 1, &d.base_off, st))) return rc;
    if ((rc = sel_stage(ctx, "sels.bases", in->bases, (size_t)n_bases, &d.bases, st))) return rc;
    if (in->quals && (rc = sel_stage(ctx, "sels.quals", in->quals, (size_t)n_bases, &d.quals, st))) return rc;
    if ((rc = sel_stage(ctx, "sels.cigar_off", in->cigar_off, (size_t)n_reads + 1, &d.cigar_off, st))) return rc;
    if ((rc = sel_stage(ctx, "sels.cigar", in->cigar, (size_t)n_cigar, &d.cigar, st))) return rc;
    if (read_hp && (rc = sel_stage(ctx, "sels.read_hp", read_hp, (size_t)n_reads, &d_hp, st))) return rc;
    pv_select_out o = *out;
    const size_t cr = (size_t)out->read_capacity, cb = (size_t)std::max<int64_t>(out->base_capacity, 1),
                 cc = (size_t)std::max<int64_t>(out->cigar_capacity, 1);
    int64_t* d_counts = nullptr;
    if ((rc = pv_get(ctx, "sels.o.read_off", (size_t)G + 1, &o.read_off))) return rc;
    if ((rc = pv_get(ctx, "sels.o.read_pos", cr + 1, &o.read_pos))) return rc;
    if ((rc = pv_get(ctx, "sels.o.read_flags", cr + 1, &o.read_flags))) return rc;
    if ((rc = pv_get(ctx, "sels.o.read_mapq", cr + 1, &o.read_mapq))) return rc;
    if ((rc = pv_get(ctx, "sels.o.base_off", cr + 1, &o.base_off))) return rc;
    if ((rc = pv_get(ctx, "sels.o.bases", cb, &o.bases))) return rc;
    if ((rc = pv_get(ctx, "sels.o.quals", cb, &o.quals))) return rc;
    if ((rc = pv_get(ctx, "sels.o.cigar_off", cr + 1, &o.cigar_off))) return rc;
    if ((rc = pv_get(ctx, "sels.o.cigar", cc, &o.cigar))) return rc;
    if (out->read_hp && (rc = pv_get(ctx, "sels.o.read_hp", cr + 1, &o.read_hp))) return rc;
    if (out->src_read && (rc = pv_get(ctx, "sels.o.src_read", cr + 1, &o.src_read))) return rc;
    if ((rc = pv_get(ctx, "sels.counts", (size_t)4, &d_counts))) return rc;
    if ((rc = pv_batch_select_hp_dev(ctx, &d, d_hp, n_reads, n_bases, n_cigar, haplotype, &o, d_counts, st))) return rc;
    int64_t counts[4];
    PV_HIP(hipMemcpyAsync(counts, d_counts, sizeof(counts), hipMemcpyDeviceToHost, st));
    PV_HIP(hipStreamSynchronize(st));
    out->n_reads = counts[0]; out->n_bases = counts[1]; out->n_cigar = counts[2];
    PV_CHECK(counts[3] != PV_ERR_INVALID, PV_ERR_INVALID, "select: malformed offsets");
    if ((rc = sel_fetch(out->read_off, o.read_off, (int64_t)G + 1, st))) return rc;
    if (counts[3] == PV_ERR_CAPACITY) {
        PV_HIP(hipStreamSynchronize(st));
        pv_set_error("select: capacity too small: need %lld reads, %lld bases, %lld cigar words", (long long)counts[0],
                     (long long)counts[1], (long long)counts[2]);
        return PV_ERR_CAPACITY;
    }
    const int64_t k = counts[0];
    if ((rc = sel_fetch(out->read_pos, o.read_pos, k, st))) return rc;
    if ((rc = sel_fetch(out->read_flags, o.read_flags, k, st))) return rc;
    if ((rc = sel_fetch(out->read_mapq, o.read_mapq, k, st))) return rc;
    if ((rc = sel_fetch(out->base_off, o.base_off, k + 1, st))) return rc;
    if ((rc = sel_fetch(out->cigar_off, o.cigar_off, k + 1, st))) return rc;
    if ((rc = sel_fetch(out->bases, o.bases, counts[1], st))) return rc;
    if (in->quals && (rc = sel_fetch(out->quals, o.quals, counts[1], st))) return rc;
    if ((rc = sel_fetch(out->cigar, o.cigar, counts[2], st))) return rc;
    if ((rc = sel_fetch(out->read_hp, o.read_hp, k, st))) return rc;
    if ((rc = sel_fetch(out->src_read, o.src_read, k, st))) return rc;
    PV_HIP(hipStreamSynchronize(st));
    return PV_OK;
}
