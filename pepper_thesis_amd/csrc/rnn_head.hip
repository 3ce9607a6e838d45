// rnn_head.hip — the head of P1 (pepper_variant) on gfx950 (MI355X), fp32 on the f32 MFMA.
//
// LSTM outputs [B,33,512] -> flatten 16896 -> 5 x (Linear 512 + SELU) -> Linear 3 -> softmax    (reference: models/simple_model.py:56-82)
//
//   k_head_splitk          linear_1 (K = 16896) as a split-K MFMA product over time-step chunks,
//        deterministic partial slabs (no float atomics).
//   k_head_tail<TR>        sum of slabs + bias + SELU, linear_2..5 + SELU (MFMA), output layer, softmax. Also the tail of the
//        chains on the bf16 MFMA for small calls (rnn_p1.hip).
// Weights come packed in MFMA fragment order (pack_linear, rnn_pack_host.hpp) through the rings of rnn_ring.hpp.
#include "rnn_f32.hpp"
#include "mfma_tiles.hpp"
#include "rnn_math.hpp"
#include "rnn_ring.hpp"

namespace {

using namespace pvdev;

constexpr int T_STEPS = PV_P1_T;
constexpr int H = PV_P1_H;        // LSTM hidden
constexpr int ROWS = PV_P1_ROWS;  // batch rows per workgroup (one MFMA M-tile)
constexpr int HEAD_N = PV_HEAD_N;
constexpr int HEAD_K = PV_HEAD_K;

struct HeadArgs {
    const float* dec;     // [B,33,512]
    const float* w1p;     // packed linear_1 [4 waves][2112 kb][4][64][4]
    float* part;          // [splits][B][512]
    int64_t B;
    int n_tiles;
    int splits;           // divides 33
    int steps_per_split;
    int per_xcd;          // > 0: XCD-aware order (see k_head_splitk); 0: tile-major order
};

__global__ __launch_bounds__(256, 1) void k_head_splitk(HeadArgs a) {
    constexpr int KC = 2 * H;  // 512 k per time step
    constexpr int LDA = KC + 4;
    extern __shared__ float smem[];
    float* abuf = smem;  // [32][LDA]
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    // XCD-aware order: workgroups are dealt round-robin to the 8 XCDs, so XCD x runs blocks x, x+8, ... Give it a
    // CONTIGUOUS range of the split-major list (split, tile): its 32 CUs then stream the same 1/splits slice of the
    // packed linear_1 weights at the same time and the slice passes through that XCD's L2 once, instead of every XCD
    // pulling all 34.6 MB for every round of tiles.
    int tile, split;
    if (a.per_xcd > 0) {
        const int l = (int)(blockIdx.x & 7) * a.per_xcd + (int)(blockIdx.x >> 3);
        if ((int)(blockIdx.x >> 3) >= a.per_xcd || l >= a.n_tiles * a.splits) return;
        split = l / a.n_tiles; tile = l - split * a.n_tiles;
    } else {
        tile = blockIdx.x / a.splits; split = blockIdx.x - tile * a.splits;
    }
    const int64_t b0 = (int64_t)tile * ROWS;
    Gate<32> acc[4];
#pragma unroll
    for (int nt = 0; nt < 4; nt++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[nt].v[r] = 0.0f;
    // this wave's slice of the packed linear_1 weights is one contiguous stream over all 33 time steps
    const __amdgpu_buffer_rsrc_t wr = make_rsrc_sized(a.w1p + (size_t)wv * (HEAD_K / 8) * 4 * 256, (unsigned)((HEAD_K / 8) * 4 * 256 * sizeof(float)));
    f32x4 bq[4][4];
    ring_prime<4>(bq, wr, split * a.steps_per_split * (KC / 8), lane);
    // A tile (32 rows x 512 of the decoder output at time step t; the buffer is padded to whole tiles) staged through
    // registers: the loads of step st+1 are issued before step st's MFMAs and written to LDS after them.
    constexpr int V4 = KC / 4, XR = ROWS * V4 / 256;   // 16 float4 per thread, rows tid/128 + 2u
    const __amdgpu_buffer_rsrc_t asr = make_rsrc(a.dec + (size_t)b0 * T_STEPS * KC);
    const unsigned a_g = (unsigned)(((tid >> 7) * T_STEPS * KC + (tid & 127) * 4) * 4);
    const unsigned a_l = (unsigned)((tid >> 7) * LDA + (tid & 127) * 4);
    f32x4 xr[XR];
    auto a_load = [&](int t) {
#pragma unroll
        for (int u = 0; u < XR; u++) xr[u] = buf_load4_nt(asr, a_g, (unsigned)((2 * u * T_STEPS + t) * KC * 4));
    };
    auto a_store = [&]() {
#pragma unroll
        for (int u = 0; u < XR; u++) *reinterpret_cast<f32x4*>(abuf + 2 * u * LDA + a_l) = xr[u];
    };
    a_load(split * a.steps_per_split);
    a_store();
    __syncthreads();
    for (int st = 0; st < a.steps_per_split; st++) {
        const int t = split * a.steps_per_split + st;
        if (st + 1 < a.steps_per_split) a_load(t + 1);
        mma_stream_ringb<32, 4>(acc, abuf, LDA, KC / 8, wr, t * (KC / 8), bq, lane);
        if (st + 1 < a.steps_per_split) {
            lds_barrier();  // every wave is done reading abuf
            a_store();
            lds_barrier();
        }
    }
    float* dst = a.part + (size_t)split * a.B * HEAD_N;
#pragma unroll
    for (int nt = 0; nt < 4; nt++) {
        const int n = 128 * wv + 32 * nt + (lane & 31);
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int64_t b = b0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (b < a.B) dst[b * HEAD_N + n] = acc[nt].v[r];
        }
    }
}

struct TailArgs {
    const float* part;   // [splits][part_rows][512]
    int splits;
    int64_t part_rows;   // rows per slab (B, or the tile-padded batch in bf16 mode)
    const float* b1;     // [512]
    const float* wp[4];  // packed linear_2..5 [4 waves][64 kb][4][64][4]
    const float* b[4];   // [512]
    const float* wo;     // [3][512]
    const float* bo;     // [3]
    float* probs;        // [B,3]
    int64_t B;
    unsigned* epoch;     // the forward-call counter of the unit-split LSTM form: bumped here, by the call's last kernel
    const int* err;      // exchange time-outs of the unit-split LSTM form since the host last acknowledged them: while it is
                         // non-zero every call's probabilities leave as NaN (both LSTM kernels of this call are complete when
                         // this kernel runs, so the word is stable here)
};

// TR = batch rows per workgroup: 32, or 16 when 32-row tiles would leave CUs idle (the tail is a chain of four dependent
// 512x512 layers per tile). wp[layer] is the packed stream of the matching tile form (pack_linear, rnn_pack_host.hpp).
template <int TR>
__global__ __launch_bounds__(256, 1) void k_head_tail(TailArgs a) {
    constexpr int LDY = HEAD_N + 4;
    constexpr int NE = TR / 2;
    extern __shared__ float smem[];
    float* y0 = smem;             // [TR][LDY]
    float* y1 = smem + TR * LDY;  // [TR][LDY]
    __shared__ float logits[TR][4];
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t b0 = (int64_t)blockIdx.x * TR;
    if (a.epoch && blockIdx.x == 0 && tid == 0) atomicAdd(a.epoch, 1u);   // both LSTM kernels of this call are done (stream order)
    // y0 = selu(sum of slabs + b1)   (simple_model.py:57-59)
    for (int i = tid; i < TR * HEAD_N; i += 256) {
        const int row = i / HEAD_N, n = i - row * HEAD_N;
        int64_t b = b0 + row;
        if (b >= a.B) b = a.B - 1;
        float v = a.b1[n];
#pragma unroll 11
        for (int s = 0; s < a.splits; s++) v += a.part[((size_t)s * a.part_rows + b) * HEAD_N + n];
        y0[row * LDY + n] = seluf_(v);
    }
    __syncthreads();
    float* src = y0;
    float* dst = y1;
    const int unit0 = 128 * wv + lane_unit<TR>(lane);  // + 32*nt + elem_unit(e)
    for (int layer = 0; layer < 4; layer++) {  // linear_2..5 + SELU (:61-76)
        Gate<TR> acc[4];
#pragma unroll
        for (int nt = 0; nt < 4; nt++)
#pragma unroll
            for (int e = 0; e < NE; e++) gate_set<TR>(acc[nt], e, a.b[layer][unit0 + 32 * nt + elem_unit<TR>(e)]);
        {
            const __amdgpu_buffer_rsrc_t wr = make_rsrc_sized(a.wp[layer] + (size_t)wv * (HEAD_N / 8) * 4 * 256,
                                                              (unsigned)((HEAD_N / 8) * 4 * 256 * sizeof(float)));
            f32x4 bq[4][4];
            ring_prime<4>(bq, wr, 0, lane);
            mma_stream_ringb<TR, 4>(acc, src, LDY, HEAD_N / 8, wr, 0, bq, lane);
        }
#pragma unroll
        for (int nt = 0; nt < 4; nt++)
#pragma unroll
            for (int e = 0; e < NE; e++)
                dst[(lane_row<TR>(lane) + elem_row<TR>(e)) * LDY + unit0 + 32 * nt + elem_unit<TR>(e)] = seluf_(gate_get<TR>(acc[nt], e));
        __syncthreads();
        float* tmp = src; src = dst; dst = tmp;
    }
    // output_layer_type (512 -> 3) + softmax(dim=1) (:77-82): 8 lanes per (row, class) pair
    {
        const int pair = tid >> 3, sub = tid & 7;  // 32 pairs per pass
        for (int p = pair; p < TR * 3; p += 32) {
            const int row = p / 3, cls = p - row * 3;
            float s = 0.0f;
            for (int k = sub; k < HEAD_N; k += 8) s += src[row * LDY + k] * a.wo[cls * HEAD_N + k];
            s += __shfl_xor(s, 4, 64);
            s += __shfl_xor(s, 2, 64);
            s += __shfl_xor(s, 1, 64);
            if (sub == 0) logits[row][cls] = s + a.bo[cls];
        }
    }
    __syncthreads();
    if (tid < TR) {
        const int64_t b = b0 + tid;
        if (b < a.B) {
            const float l0 = logits[tid][0], l1 = logits[tid][1], l2 = logits[tid][2];
            const float m = fmaxf(l0, fmaxf(l1, l2));
            const float e0 = expf(l0 - m), e1 = expf(l1 - m), e2 = expf(l2 - m);
            const float inv = 1.0f / (e0 + e1 + e2);
            // a poll of the unit-split form gave up (a partner workgroup was not resident): the numbers below are computed from
            // stale hidden state. They must not look like results: NaN until the host acknowledges (pv_rnn_exchange_timeouts).
            const bool bad = a.err && a.err[0] != 0;
            const float nanv = __builtin_nanf("");
            a.probs[b * 3 + 0] = bad ? nanv : e0 * inv;
            a.probs[b * 3 + 1] = bad ? nanv : e1 * inv;
            a.probs[b * 3 + 2] = bad ? nanv : e2 * inv;
        }
    }
}

constexpr size_t LDS_SPLITK = (size_t)ROWS * (2 * H + 4) * sizeof(float);
template <int TR> constexpr size_t lds_tail() { return (size_t)2 * TR * (HEAD_N + 4) * sizeof(float); }

}  // namespace

int pv_head_f32_prepare() {
    // opt in to > 64 KB of dynamic LDS (exact sizes; static LDS counts against the 160 KB too)
    PV_HIP(hipFuncSetAttribute((const void*)k_head_splitk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_SPLITK));
    PV_HIP(hipFuncSetAttribute((const void*)k_head_tail<32>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_tail<32>()));
    PV_HIP(hipFuncSetAttribute((const void*)k_head_tail<16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_tail<16>()));
    return PV_OK;
}

int pv_head_splitk_async(pv_ctx* ctx, const pv_head_splitk_desc& d, hipStream_t st) {
    HeadArgs h;
    h.dec = d.dec; h.w1p = d.w1p; h.part = d.part; h.B = d.B; h.n_tiles = d.n_tiles; h.splits = d.splits; h.steps_per_split = T_STEPS / d.splits;
    const int total_wg = d.n_tiles * d.splits;
    h.per_xcd = d.head_map ? (total_wg + 7) / 8 : 0;
    const unsigned head_grid = d.head_map ? (unsigned)(h.per_xcd * 8) : (unsigned)total_wg;
    pv_prof_scope ps(ctx, "k_head_splitk", st);
    k_head_splitk<<<head_grid, 256, LDS_SPLITK, st>>>(h);
    return PV_OK;
}

int pv_head_tail_async(pv_ctx* ctx, const pv_head_tail_desc& d, hipStream_t st) {
    const int n_tiles32 = (int)((d.B + ROWS - 1) / ROWS);
    TailArgs t;
    t.part = d.part; t.b1 = d.b1; t.splits = d.splits; t.part_rows = d.part_rows;
    t.wo = d.wo; t.bo = d.bo; t.probs = d.probs; t.B = d.B; t.epoch = d.epoch; t.err = d.err;
    for (int i = 0; i < 4; i++) { t.wp[i] = d.wp[i]; t.b[i] = d.b[i]; }
    pv_prof_scope ps(ctx, "k_head_tail", st);
    if (d.rows == 32) k_head_tail<32><<<(unsigned)n_tiles32, 256, lds_tail<32>(), st>>>(t);
    else k_head_tail<16><<<(unsigned)(2 * n_tiles32), 256, lds_tail<16>(), st>>>(t);
    return PV_OK;
}
