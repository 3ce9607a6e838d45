// polish_qual.hip — the polisher's per-base quality: P2 labels + accumulated softmax -> one Phred byte per chunk row.
//
// The rule (include/pepper_hip.h, pv_polish_row_qual) restates what the reference's caller meant to compute,
// -10 log10(1 - value / counts) per column (pepper/modules/python/models/predict_distributed_gpu.py:96-105, which feeds the
// label in place of the value), as a count of literal thresholds (polish_qual_table.hpp) so that host and device agree bit
// for bit: for row r of a chunk, cnt = 1 on the seq_overlap rows at either end and 2 elsewhere (the windows that cover the
// row), err = 1 - acc[r][label[r]] / cnt in float32, q = #{k in 1..93 : err <= T[k]}.
//
// Two launches, no global atomics: one lane per row over blocks of 256 rows (the block's 5120 bytes of acc staged through
// LDS with 16-byte loads: a lane's own 20-byte stride would waste three quarters of every request), each block leaving its
// first row with a label above 4; then one block folding those into d_counts.
#include "polish_qual_table.hpp"
#include "pv_common.hpp"

namespace {

constexpr int RQ_THREADS = 256;
constexpr int RQ_STATUS_THREADS = 1024;

__constant__ float c_qual_t[PV_QUAL_MAX + 1] = {PV_QUAL_T_VALUES};
const float h_qual_t[PV_QUAL_MAX + 1] = {PV_QUAL_T_VALUES};

// block minimum; NT threads, NT/64 waves
template <int NT, typename T>
__device__ inline T block_min(T v, T* lds) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const T y = __shfl_xor(v, d, 64);
        v = y < v ? y : v;
    }
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    T m = lds[0];
#pragma unroll
    for (int i = 1; i < NT / 64; i++) m = lds[i] < m ? lds[i] : m;
    return m;
}

// one lane per row; wide: acc is 16-byte aligned (a block starts 5120 * blockIdx.x bytes into it)
__global__ __launch_bounds__(RQ_THREADS) void k_row_qual(const uint8_t* __restrict__ lab, const float* __restrict__ acc,
                                                         int64_t n_rows, int L, int O, int wide, uint8_t* __restrict__ qual,
                                                         int32_t* __restrict__ blk_bad) {
#pragma clang fp contract(off)
    __shared__ float s_t[PV_QUAL_MAX + 1];
    __shared__ __attribute__((aligned(16))) float s_acc[RQ_THREADS * 5];
    __shared__ int32_t s_min[RQ_THREADS / 64];
    const int64_t row0 = (int64_t)blockIdx.x * RQ_THREADS;
    const int rows = (int)min<int64_t>(RQ_THREADS, n_rows - row0);
    const int nf = rows * 5;
    const float* src = acc + row0 * 5;
    if (threadIdx.x <= PV_QUAL_MAX) s_t[threadIdx.x] = c_qual_t[threadIdx.x];
    int first = 0;
    if (wide) {
        const int n4 = nf >> 2;
        for (int i = threadIdx.x; i < n4; i += RQ_THREADS)
            reinterpret_cast<float4*>(s_acc)[i] = reinterpret_cast<const float4*>(src)[i];
        first = n4 << 2;
    }
    for (int i = first + threadIdx.x; i < nf; i += RQ_THREADS) s_acc[i] = src[i];
    __syncthreads();
    int32_t bad = INT32_MAX;
    if ((int)threadIdx.x < rows) {
        const int64_t t = row0 + threadIdx.x;
        const int r = (int)(t % L);
        const int lb = lab[t];
        int q = 0;
        if (lb > 4) {
            bad = (int32_t)threadIdx.x;
        } else {
            const float cnt = (r < O || r >= L - O) ? 1.0f : 2.0f;
            const float err = 1.0f - s_acc[threadIdx.x * 5 + lb] / cnt;   // (the lanes' stride of 5 dwords spreads over the banks)
            // T decreases, so the count is the largest k with err <= T[k]: 7 steps over 1..93; a NaN passes none
#pragma unroll
            for (int s = 64; s >= 1; s >>= 1) {
                const int k = q + s;
                if (k <= PV_QUAL_MAX && err <= s_t[k <= PV_QUAL_MAX ? k : PV_QUAL_MAX]) q = k;
            }
        }
        qual[t] = (uint8_t)q;
    }
    const int32_t m = block_min<RQ_THREADS, int32_t>(bad, s_min);
    if (threadIdx.x == 0) blk_bad[blockIdx.x] = m == INT32_MAX ? -1 : m;
}

// one block: the first row with a label above 4 over all blocks -> d_counts
__global__ __launch_bounds__(RQ_STATUS_THREADS) void k_row_qual_status(const int32_t* __restrict__ blk_bad, int64_t n_blocks,
                                                                       int64_t n_rows, int L, int64_t* __restrict__ counts) {
    __shared__ int64_t s_min[RQ_STATUS_THREADS / 64];
    int64_t bad = INT64_MAX;
    for (int64_t i = threadIdx.x; i < n_blocks; i += RQ_STATUS_THREADS)
        if (blk_bad[i] >= 0 && bad == INT64_MAX) bad = i * RQ_THREADS + blk_bad[i];
    const int64_t m = block_min<RQ_STATUS_THREADS, int64_t>(bad, s_min);
    if (threadIdx.x == 0) {
        counts[0] = n_rows;
        counts[1] = m == INT64_MAX ? PV_OK : PV_ERR_STATE;
        counts[2] = m == INT64_MAX ? -1 : m / L;
        counts[3] = m == INT64_MAX ? 0 : m % L;
    }
}

}  // namespace

extern "C" float pv_polish_qual_threshold(int k) { return k >= 0 && k <= PV_QUAL_MAX ? h_qual_t[k] : 0.0f; }

extern "C" int pv_polish_row_qual_dev(pv_ctx* ctx, const uint8_t* labels, const float* acc, int64_t B, int seq_length,
                                      int seq_overlap, uint8_t* qual, int64_t* d_counts, void* stream) {
    PV_CHECK(ctx && d_counts, PV_ERR_INVALID, "null argument");
    PV_CHECK(B >= 0, PV_ERR_INVALID, "negative sizes");
    PV_CHECK(seq_length >= 1 && seq_overlap >= 0 && 2 * (int64_t)seq_overlap <= seq_length, PV_ERR_INVALID,
             "row quality: need seq_length >= 1 and 0 <= 2 * seq_overlap <= seq_length (got %d, %d)", seq_length, seq_overlap);
    PV_CHECK(B < (1ll << 31), PV_ERR_LIMIT, "too many chunks for one launch");
    const int64_t n_rows = B * seq_length;
    const int64_t n_blocks = (n_rows + RQ_THREADS - 1) / RQ_THREADS;
    PV_CHECK(n_blocks < (1ll << 31), PV_ERR_LIMIT, "too many rows for one launch");
    PV_CHECK(B == 0 || (labels && acc && qual), PV_ERR_INVALID, "labels, acc or qual missing");
    PV_CHECK(((uintptr_t)acc & 3) == 0, PV_ERR_INVALID, "acc is not aligned to a float");
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = pv_pick_stream(ctx, stream);
    int32_t* blk_bad = nullptr;
    int rc;
    if ((rc = pv_get(ctx, "rowqual.bad", (size_t)(n_blocks > 0 ? n_blocks : 1), &blk_bad))) return rc;
    pv_prof_scope ps_all(ctx, "polish_row_qual", st);
    if (n_blocks > 0) {
        pv_prof_scope ps(ctx, "k_row_qual", st);
        k_row_qual<<<(unsigned)n_blocks, RQ_THREADS, 0, st>>>(labels, acc, n_rows, seq_length, seq_overlap,
                                                              ((uintptr_t)acc & 15) == 0, qual, blk_bad);
    }
    k_row_qual_status<<<1, RQ_STATUS_THREADS, 0, st>>>(blk_bad, n_blocks, n_rows, seq_length, d_counts);
    PV_HIP(hipGetLastError());
    return PV_OK;
}

extern "C" int pv_polish_row_qual(pv_ctx* ctx, const uint8_t* labels, const float* acc, int64_t B, int seq_length, int seq_overlap,
                                  uint8_t* qual, int64_t* counts) {
    PV_CHECK(ctx && counts, PV_ERR_INVALID, "null argument");
    PV_CHECK(B >= 0 && seq_length >= 1, PV_ERR_INVALID, "negative sizes");
    PV_CHECK(B == 0 || (labels && acc && qual), PV_ERR_INVALID, "labels, acc or qual missing");
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)B * (size_t)seq_length;
    uint8_t *d_lab = nullptr, *d_qual = nullptr;
    float* d_acc = nullptr;
    int64_t* d_counts = nullptr;
    int rc;
    if ((rc = pv_get(ctx, "rq.labels", n > 0 ? n : 1, &d_lab))) return rc;
    if ((rc = pv_get(ctx, "rq.acc", n > 0 ? n * 5 : 1, &d_acc))) return rc;
    if ((rc = pv_get(ctx, "rq.qual", n > 0 ? n : 1, &d_qual))) return rc;
    if ((rc = pv_get(ctx, "rq.counts", (size_t)4, &d_counts))) return rc;
    if (n > 0) {
        PV_HIP(hipMemcpyAsync(d_lab, labels, n, hipMemcpyHostToDevice, st));
        PV_HIP(hipMemcpyAsync(d_acc, acc, n * 5 * sizeof(float), hipMemcpyHostToDevice, st));
    }
    rc = pv_polish_row_qual_dev(ctx, d_lab, d_acc, B, seq_length, seq_overlap, d_qual, d_counts, st);
    if (rc) return rc;
    PV_HIP(hipMemcpyAsync(counts, d_counts, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (n > 0) PV_HIP(hipMemcpyAsync(qual, d_qual, n, hipMemcpyDeviceToHost, st));
    PV_HIP(hipStreamSynchronize(st));
    PV_CHECK(counts[1] != PV_ERR_STATE, PV_ERR_STATE,
             "row quality: chunk %lld, row %lld holds a label outside 0..4 (a poisoned network result)", (long long)counts[2],
             (long long)counts[3]);
    PV_CHECK(counts[1] == PV_OK, (int)counts[1], "row quality: device status %lld", (long long)counts[1]);
    return PV_OK;
}
