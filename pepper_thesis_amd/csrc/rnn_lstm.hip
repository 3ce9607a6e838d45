// rnn_lstm.hip — the LSTM layers of P1 (pepper_variant) on gfx950 (MI355X), fp32 on the f32 MFMA.
//
// images int8 [B,33,26] -> bi-LSTM(256) -> bi-LSTM(256)      (reference: models/simple_model.py:48-54; the head: rnn_head.hip)
//
//   k_lstm_layer<KP,INT8,TR>  one launch per LSTM layer; a workgroup (8 waves) = (TR-row batch tile, direction). Per
//        time step the gate pre-activations [TR x 1024] = [x_t | h_{t-1}] . [W_ih | W_hh]^T are ONE concatenated-K
//        product on the f32 MFMA (bitwise an fmaf chain), so the "input-projection GEMM" and the recurrent product
//        share accumulators and no pre-activation tensor ever goes to HBM. A operand (x_t, h_{t-1}) lives in LDS; the
//        B operand (weights) is pre-packed on the host in exact MFMA fragment order (pack_lstm, rnn_pack_host.hpp) and
//        streamed from L2 through a four-deep register ring (rnn_ring.hpp) fed by raw buffer loads three k-blocks ahead;
//        wave w owns hidden units [32w, 32w+32) of all four gates so the cell update is purely in-register. c stays in
//        registers for all 33 steps, h is exchanged between the waves through a double-buffered LDS tile. XCD-aware block
//        mapping keeps one direction's weights (<= 3 MB) per XCD L2. Two tile forms (mfma_tiles.hpp): TR = 32 on 32x32x2
//        MFMAs when the workgroups fill the chip, TR = 16 on 16x16x4 MFMAs below that.
//   k_lstm_split<KP,INT8,NS>  the unit-split form for ONE small batch on the whole chip (below).
#include "rnn_f32.hpp"
#include "mfma_tiles.hpp"
#include "rnn_math.hpp"
#include "rnn_ring.hpp"

namespace {

using namespace pvdev;

constexpr int T_STEPS = PV_P1_T;
constexpr int F_IN = PV_P1_F;
constexpr int H = PV_P1_H;        // LSTM hidden
constexpr int ROWS = PV_P1_ROWS;  // the 32-row tile the launch is counted in

// x tiles and layer outputs are touched once: streaming (nt) forms, so that the packed weights (3.1 MB per direction in a
// 4 MB L2) stay resident. rocprofv3 FETCH_SIZE of the decoder: 664 MB per launch without the hint (weights re-fetched on
// every time step), 299 MB with it (= the 277 MB x tensor + weights); run time unchanged (the misses were Infinity Cache hits).
#define PV_XLOAD buf_load4_nt
#define PV_OSTORE buf_store1_nt

struct LstmArgs {
    const int8_t* x_i8;   // [B,33,26]    (encoder)
    const float* x_f32;   // [Bp,33,512]  (decoder; padded to whole 32-row tiles)
    const float* wp;      // packed [2 dirs][8 waves][nkb][4 gates][64][4] in the tile form of the launch
    const float* bias;    // [2][1024] b_ih + b_hh
    float* out;           // [Bp,33,512] fp32
    int64_t B;
    int n_tiles;          // tiles of TR rows
};

// One LSTM layer. KP = padded input width (multiple of 32): 32 for the encoder (26 real, from int8), 512 for the decoder.
// TR = batch rows per workgroup (mfma_tiles.hpp). Workgroup = (batch tile, direction), 8 waves (two per SIMD: one wave's
// LDS/L2 waits and cell update hide behind the other's MFMAs); wave w owns hidden units [32w, 32w+32) of the four gates.
template <int KP, bool INT8, int TR>
__global__ __launch_bounds__(512, 2) void k_lstm_layer(LstmArgs a) {
    constexpr int LDX = KP + 4, LDH = H + 4;
    constexpr int NKB_X = KP / 8, NKB_H = H / 8;
    constexpr int NT = 4;         // gates i, f, g, o
    constexpr int NE = TR / 2;    // accumulator elements per lane per gate
    constexpr int NTHR = 512;
    static_assert((NKB_X + NKB_H) % 4 == 0, "mma_dual_ringb works in groups of four k-blocks");
    extern __shared__ float smem[];
    float* xbuf = smem;               // [TR][LDX]
    float* hbuf = smem + TR * LDX;    // [2][TR][LDH]
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);  // SGPR: bases/offsets derived from it stay scalar
    // XCD-aware mapping: blocks b and b+8 share an XCD (round-robin dispatch); give every XCD one
    // direction only so that its L2 holds a single direction's packed weights.
    const int xcd = blockIdx.x & 7;
    const int dir = xcd & 1;
    const int tile = (blockIdx.x >> 3) * 4 + (xcd >> 1);
    if (tile >= a.n_tiles) return;
    const int64_t b0 = (int64_t)tile * TR;
    const float* wp = a.wp + ((size_t)(dir * 8 + wv) * (NKB_X + NKB_H)) * NT * 256;
    const float* bias = a.bias + dir * 4 * H;

    for (int i = tid; i < 2 * TR * LDH; i += NTHR) hbuf[i] = 0.0f;
    float cst[NE];
#pragma unroll
    for (int e = 0; e < NE; e++) cst[e] = 0.0f;
    const int unit0 = 32 * wv + lane_unit<TR>(lane);
    float bs[NT][TR == 32 ? 1 : 2];
#pragma unroll
    for (int nt = 0; nt < NT; nt++)
#pragma unroll
        for (int t2 = 0; t2 < (TR == 32 ? 1 : 2); t2++) bs[nt][t2] = bias[nt * H + unit0 + 16 * t2];
    const __amdgpu_buffer_rsrc_t wr = make_rsrc(wp);
    f32x4 bq[4][NT];
    ring_prime<NT>(bq, wr, 0, lane);

    // x_t staging through registers: the loads for step s+1 are issued before step s's MFMAs and written to LDS after
    // them, so their latency hides behind the matrix work.
    constexpr int V4 = KP / 4;                            // float4 per row (fp32 input)
    constexpr int XR = INT8 ? 1 : TR * V4 / NTHR;         // decoder: float4 per thread, rows tid/128 + 4u
    constexpr int XI = INT8 ? TR * KP / NTHR : 1;         // encoder: floats per thread, rows tid/32 + 16u
    f32x4 xr[XR];
    unsigned xi[XI];                                      // raw bytes: converted when written to LDS (a conversion right behind
                                                          // the load would make hipcc drain the vmcnt queue, ring included, per step)
    int xoff[XI];                                         // encoder: offset of (row's window, feature k) from the tile's first window
                                                          // (negative when a 16-row half tile lies wholly beyond B)
    // the decoder input is padded to whole 32-row tiles (rows beyond B replicate row B-1): no clamp, and the address is
    // (tile resource) + (lane offset, computed once) + (scalar offset of row group u and step t)
    const __amdgpu_buffer_rsrc_t xsr = make_rsrc(INT8 ? (const void*)a.wp : (const void*)(a.x_f32 + (size_t)b0 * T_STEPS * KP));
    const __amdgpu_buffer_rsrc_t osr = make_rsrc(a.out + (size_t)b0 * T_STEPS * 2 * H);
    const unsigned xg_l = (unsigned)(((tid / V4) * T_STEPS * KP + (tid % V4) * 4) * 4);
    const unsigned xl_l = (unsigned)((tid / V4) * LDX + (tid % V4) * 4);
    const unsigned xe_l = (unsigned)((tid >> 5) * LDX + (tid & 31));
    const bool xe_valid = (tid & 31) < F_IN;
    if constexpr (INT8) {
        static_assert(KP == 32, "encoder staging assumes 32 padded features");
#pragma unroll
        for (int u = 0; u < XI; u++) {
            int64_t r = (tid >> 5) + 16 * u;
            if (b0 + r >= a.B) r = a.B - 1 - b0;   // rows beyond B replicate row B-1 (finite values; never stored to the caller)
            xoff[u] = (int)(r * T_STEPS * F_IN) + ((tid & 31) < F_IN ? (tid & 31) : F_IN - 1);   // padding lanes re-read feature 25
        }
    }
    const int8_t* img0 = a.x_i8 + (size_t)b0 * T_STEPS * F_IN;  // uniform
    auto x_load = [&](int t) {
        if constexpr (INT8) {
            const int8_t* src = img0 + t * F_IN;
#pragma unroll
            for (int u = 0; u < XI; u++) xi[u] = (unsigned)(int)src[xoff[u]];
        } else {
#pragma unroll
            for (int u = 0; u < XR; u++) xr[u] = PV_XLOAD(xsr, xg_l, (unsigned)(((u * (NTHR / V4)) * T_STEPS + t) * KP * 4));
        }
    };
    auto x_store = [&]() {
        if constexpr (INT8) {
#pragma unroll
            for (int u = 0; u < XI; u++) (xbuf + u * 16 * LDX)[xe_l] = xe_valid ? (float)(int)xi[u] : 0.0f;
        } else {
#pragma unroll
            for (int u = 0; u < XR; u++) *reinterpret_cast<f32x4*>(xbuf + u * (NTHR / V4) * LDX + xl_l) = xr[u];
        }
    };
    const unsigned h_l = (unsigned)(lane_row<TR>(lane) * LDH + unit0);                      // lane part of the h tile offset
    const unsigned og_l = (unsigned)((lane_row<TR>(lane) * T_STEPS * 2 * H + unit0) * 4);   // lane part of the output byte offset
    x_load(dir ? T_STEPS - 1 : 0);
    x_store();
    __syncthreads();

    for (int s = 0; s < T_STEPS; s++) {
        const int t = dir ? (T_STEPS - 1 - s) : s;
        const int cur = s & 1, nxt = cur ^ 1;
        if (s + 1 < T_STEPS) x_load(dir ? (T_STEPS - 2 - s) : (s + 1));
        // ---- gates = bias + [x_t | h_{t-1}] . [W_ih | W_hh]^T -------------------------------------
        Gate<TR> acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; nt++)
#pragma unroll
            for (int e = 0; e < NE; e++) gate_set<TR>(acc[nt], e, bs[nt][TR == 32 ? 0 : e >> 2]);
        // h_0 = 0 (simple_model.py:50-54 passes no initial state): the recurrent product of the first step is zero, skip it
        static_assert(NKB_X % 4 == 0, "the x-only first step needs whole groups of four k-blocks");
        mma_dual_ringb<TR, NT>(acc, xbuf, LDX, NKB_X, hbuf + cur * TR * LDH, LDH, s == 0 ? 0 : NKB_H, wr, bq, lane);
        // ---- cell update (PyTorch gate order i,f,g,o) ----------------------------------------------
        float* hn = hbuf + nxt * TR * LDH;
#pragma unroll
        for (int e = 0; e < NE; e++) {
            const float ig = sigmoidf_(gate_get<TR>(acc[0], e));
            const float fg = sigmoidf_(gate_get<TR>(acc[1], e));
            const float gg = tanhf_fma_(gate_get<TR>(acc[2], e));
            const float og = sigmoidf_(gate_get<TR>(acc[3], e));
            const float c = lstm_c_(fg, cst[e], ig, gg);
            cst[e] = c;
            const float h = og * tanhf_fma_(c);
            (hn + elem_row<TR>(e) * LDH + elem_unit<TR>(e))[h_l] = h;
            // outputs are padded to whole tiles: unconditional stores, tile resource + lane offset + scalar offset
            const unsigned o_s = (unsigned)((t * 2 * H + dir * H + elem_row<TR>(e) * T_STEPS * 2 * H + elem_unit<TR>(e)) * 4);
            PV_OSTORE(h, osr, og_l, o_s);
        }
        lds_barrier();  // everyone is done reading xbuf / hbuf[cur]; hbuf[nxt] is complete (LDS only: mfma_tiles.hpp)
        if (s + 1 < T_STEPS) {
            x_store();
            lds_barrier();
        }
    }
}


// ---- unit-split form of the LSTM layer: ONE small batch on the whole chip ----------------------------------------------
// A single 512-window call is 32 tiles of 16 rows x 2 directions = 64 workgroups of the form above on 256 CUs, and a launch
// is a chain of 33 dependent steps whose length is the per-step MFMA time of ONE workgroup. Here the 256 hidden units of a
// (tile, direction) are split over SP_NS = 4 workgroups of 4 waves (one per SIMD); a wave owns 16 units x 4 gates (one
// 16x16 accumulator per gate), so a step costs a quarter of the MFMA cycles. What the split costs is one exchange per step:
// every workgroup needs all 256 values of h_t for the recurrent product of step t+1. It is hidden behind the x-part of that
// step, which does not depend on h_t (two thirds of the decoder's MFMAs), and it needs no flag, fence or store drain:
//   * h leaves a lane as DATA-TAGGED 8-byte pairs {h(row r), tag}, tag = launch base + step + 1, two pairs per 16-byte
//     store, written through (sc1) to slot (step parity) of the exchange buffer; an aligned 8-byte pair lands whole;
//   * after its x-part MFMAs of the next step every thread reads the granules of the same thread of the three partner
//     workgroups with L1-bypassing (sc1) loads until their tags match (bounded), and writes them to the h tile in LDS.
//   A workgroup overwrites slot p two steps later; by then it has consumed every partner's granules of the step in between,
//   which a partner only writes after reading slot p. (PV_SPLIT_FENCES builds the counter + agent-scope release / acquire
//   form of the same exchange: 1.15 instead of 0.9x ms per 512-window call.)
// Used only while every workgroup of the launch can be resident at once (grid <= CUs).
// Weight stream of a wave: [k-block of 8][2][lane][4] = {i j0, i j1, f j0, f j1}, {g j0, g j1, o j0, o j1} with
// W[gate*H + 64*part + 16*wave + (lane&15)][8kb + 2*(lane>>4) + j], K = [x (padded) | h] (pack_lstm_split, rnn_pack_host.hpp), through a ring of SP_D register
// sets requested SP_D-1 k-blocks ahead (a k-block is only 8 MFMAs = 256 cycles and nothing else hides L2 latency with one
// wave per SIMD); the ring wraps into the next step.
constexpr int SP_D = 12;
// NS = workgroups per (tile, direction): 4 (4 waves each, up to 512 windows on 256 CUs) or 2 (8 waves each, two per SIMD,
// up to 1024 windows). NS * threads per workgroup = 1024 in both, so the exchange buffer has one shape.
constexpr int SP_FLAG_STRIDE = 32;   // ints between two counters: every counter on a 128-byte line of its own (fence form)
constexpr int SP_SC1 = 16;           // cache policy bit 4 = sc1 on gfx94x / gfx950: write-through stores, L1-bypassing loads
constexpr int SP_HX_QUADS = 2 * 2 * 1024;          // 16-byte granules per (tile, direction): [2 slots][NS parts][2][1024 / NS threads]

struct LstmSplitArgs {
    const int8_t* x_i8;   // [B,33,26]    (encoder)
    const float* x_f32;   // [Bp,33,512]  (decoder)
    const float* wp;      // packed [2 dirs][NS parts][16 / NS waves][nkb][2][64][4]
    const float* bias;    // [2][1024]
    float* out;           // [Bp,33,512]
    u32x4* hx;            // [n_tiles*2][SP_HX_QUADS] tagged h granules
    int* flags;           // [n_tiles*2][4 parts][SP_FLAG_STRIDE] (fence form only)
    int64_t B;
    int n_tiles;          // 16-row tiles
    const unsigned* epoch;  // device word, bumped once per forward call by its last kernel (k_head_tail): tags of this launch run
    int layer;              // from (2 * epoch + layer) * 64 + 1, so a replayed hipGraph advances them like eager launches do
    int* err;             // bumped when a bounded poll of the exchange gave up (a partner workgroup never showed up)
    int spin_limit;       // polls give up after this many tries (pv_opts::exchange_spin_log2)
    int drop_part;        // diagnostic (pv_opts::debug_drop_part): the workgroups of this part leave at once; -1 = none
};

template <int KB0, int NKB, int NTOT>
__device__ __forceinline__ void ring_split(f32x4 (&acc)[4], const float* __restrict__ A, int lda, __amdgpu_buffer_rsrc_t wr,
                                           f32x4 (&bq)[SP_D][2], int lane) {
    static_assert(NTOT % SP_D == 0, "ring depth must divide the stream length");
    const float* ap = afrag_ptr<16>(A, lda, lane);
    const unsigned lane16 = (unsigned)lane * 16u;
    f32x2 aq[2];
    aq[0] = *reinterpret_cast<const f32x2*>(ap);
#pragma unroll
    for (int i = 0; i < NKB; i++) {
        {   // request block i + SP_D - 1 (wrapping into the next step's first blocks)
            const int kbv = (KB0 + i + SP_D - 1) % NTOT;
            const int slot = (KB0 + i + SP_D - 1) % SP_D;
            bq[slot][0] = buf_load4(wr, lane16, (unsigned)((kbv * 2 + 0) * 1024));
            bq[slot][1] = buf_load4(wr, lane16, (unsigned)((kbv * 2 + 1) * 1024));
        }
        if (i + 1 < NKB) aq[(i + 1) & 1] = *reinterpret_cast<const f32x2*>(ap + 8 * (i + 1));
        __builtin_amdgcn_sched_barrier(0);
        {   // j outer, gate inner: an accumulator is reused only after three other MFMAs
            const int slot = (KB0 + i) % SP_D;
            const f32x2 av = aq[i & 1];
#pragma unroll
            for (int j = 0; j < 2; j++) {
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], bq[slot][0][j], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], bq[slot][0][2 + j], acc[1], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], bq[slot][1][j], acc[2], 0, 0, 0);
                acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], bq[slot][1][2 + j], acc[3], 0, 0, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

template <int KP, bool INT8, int SP_NS>
__global__ __launch_bounds__(1024 / SP_NS) void k_lstm_split(LstmSplitArgs a) {
    constexpr int TR = 16, LDX = KP + 4, LDH = H + 4;
    constexpr int NKB_X = KP / 8, NKB_H = H / 8, NTOT = NKB_X + NKB_H;
    constexpr int NTHR = 1024 / SP_NS, NW = NTHR / 64, UPP = H / SP_NS;   // threads, waves, units per part
    extern __shared__ float smem[];
    float* xbuf = smem;               // [16][LDX]
    float* hbuf = smem + TR * LDX;    // [2][16][LDH]: all 256 units of h
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    // the four parts of a (tile, direction) sit on ONE XCD (they exchange through its L2), one direction per XCD
    const int xcd = blockIdx.x & 7, q = blockIdx.x >> 3;
    const int part = q % SP_NS;
    const int dir = xcd & 1;
    const int tile = (q / SP_NS) * 4 + (xcd >> 1);
    if (tile >= a.n_tiles) return;   // whole groups leave together: `tile` does not depend on `part`
    if (part == a.drop_part) return; // diagnostic: a partner that never shows up (its twins' polls time out and say so)
    const int td = tile * 2 + dir;
    const int64_t b0 = (int64_t)tile * TR;
    const float* wp = a.wp + ((size_t)((dir * SP_NS + part) * NW + wv) * NTOT) * 2 * 256;
    const float* bias = a.bias + dir * 4 * H;
    const unsigned flag_base = (a.epoch[0] * 2u + (unsigned)a.layer) * 64u;   // unsigned wrap-around is harmless: tags are compared for equality
    const int unit = UPP * part + 16 * wv + (lane & 15);
    const int rowg = lane >> 4;       // this lane holds rows 4*rowg .. 4*rowg+3 of its unit

    for (int i = tid; i < 2 * TR * LDH; i += NTHR) hbuf[i] = 0.0f;
    float cst[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float bs[4];
#pragma unroll
    for (int g = 0; g < 4; g++) bs[g] = bias[g * H + unit];
    const __amdgpu_buffer_rsrc_t wr = make_rsrc(wp);
    f32x4 bq[SP_D][2];
#pragma unroll
    for (int k = 0; k < SP_D - 1; k++) {
        bq[k][0] = buf_load4(wr, (unsigned)lane * 16u, (unsigned)((k * 2 + 0) * 1024));
        bq[k][1] = buf_load4(wr, (unsigned)lane * 16u, (unsigned)((k * 2 + 1) * 1024));
    }

    // x_t staging through registers (as in k_lstm_layer): every part loads the whole 16-row x tile
    constexpr int V4 = KP / 4;
    constexpr int XR = INT8 ? 1 : TR * V4 / NTHR;   // decoder: 8 (4) float4 per thread, rows tid/128 + (NTHR/128) u
    constexpr int XI = INT8 ? TR * KP / NTHR : 1;   // encoder: 2 (1) bytes per thread, rows tid/32 + (NTHR/32) u
    constexpr int XRS = NTHR / 32;                  // encoder row stride between a thread's elements
    f32x4 xr[XR];
    unsigned xi[XI];
    int xoff[XI];
    const __amdgpu_buffer_rsrc_t xsr = make_rsrc(INT8 ? (const void*)a.wp : (const void*)(a.x_f32 + (size_t)b0 * T_STEPS * KP));
    const __amdgpu_buffer_rsrc_t osr = make_rsrc(a.out + (size_t)b0 * T_STEPS * 2 * H);
    const unsigned xg_l = (unsigned)(((tid / V4) * T_STEPS * KP + (tid % V4) * 4) * 4);
    const unsigned xl_l = (unsigned)((tid / V4) * LDX + (tid % V4) * 4);
    const unsigned xe_l = (unsigned)((tid >> 5) * LDX + (tid & 31));
    const bool xe_valid = (tid & 31) < F_IN;
    if constexpr (INT8) {
        static_assert(KP == 32, "encoder staging assumes 32 padded features");
#pragma unroll
        for (int u = 0; u < XI; u++) {
            int64_t r = (tid >> 5) + XRS * u;
            if (b0 + r >= a.B) r = a.B - 1 - b0;   // rows beyond B replicate row B-1
            xoff[u] = (int)(r * T_STEPS * F_IN) + ((tid & 31) < F_IN ? (tid & 31) : F_IN - 1);
        }
    }
    const int8_t* img0 = a.x_i8 + (size_t)b0 * T_STEPS * F_IN;
    auto x_load = [&](int t) {
        if constexpr (INT8) {
            const int8_t* src = img0 + t * F_IN;
#pragma unroll
            for (int u = 0; u < XI; u++) xi[u] = (unsigned)(int)src[xoff[u]];
        } else {
#pragma unroll
            for (int u = 0; u < XR; u++) xr[u] = PV_XLOAD(xsr, xg_l, (unsigned)(((u * (NTHR / V4)) * T_STEPS + t) * KP * 4));
        }
    };
    auto x_store = [&]() {
        if constexpr (INT8) {
#pragma unroll
            for (int u = 0; u < XI; u++) (xbuf + u * XRS * LDX)[xe_l] = xe_valid ? (float)(int)xi[u] : 0.0f;
        } else {
#pragma unroll
            for (int u = 0; u < XR; u++) *reinterpret_cast<f32x4*>(xbuf + u * (NTHR / V4) * LDX + xl_l) = xr[u];
        }
    };
    const unsigned h_l = (unsigned)(4 * rowg * LDH + unit);
    const unsigned og_l = (unsigned)((4 * rowg * T_STEPS * 2 * H + unit) * 4);
    const __amdgpu_buffer_rsrc_t hsr = make_rsrc(a.hx + (size_t)td * SP_HX_QUADS);
    // granule (slot, part, g) of thread tid: 16-byte index ((slot * SP_NS + part) * 2 + g) * NTHR + tid
    auto hx_off = [](int slot, int prt, int g) { return (unsigned)((((slot * SP_NS + prt) * 2 + g) * NTHR) * 16); };
#ifdef PV_SPLIT_FENCES
    int* flags_td = a.flags + (size_t)td * SP_NS * SP_FLAG_STRIDE;
#endif
    x_load(dir ? T_STEPS - 1 : 0);
    x_store();
    __syncthreads();

    for (int s = 0; s < T_STEPS; s++) {
        const int t = dir ? (T_STEPS - 1 - s) : s;
        const int cur = s & 1, nxt = cur ^ 1;
        if (s + 1 < T_STEPS) x_load(dir ? (T_STEPS - 2 - s) : (s + 1));
        f32x4 acc[4];
#pragma unroll
        for (int g = 0; g < 4; g++) acc[g] = f32x4{bs[g], bs[g], bs[g], bs[g]};
        ring_split<0, NKB_X, NTOT>(acc, xbuf, LDX, wr, bq, lane);          // x-part: independent of h_{t-1}
        if (s > 0) {
            // ---- the other three quarters of h_{t-1}: the granules of this thread's twins in the partner workgroups ----
            const unsigned want = flag_base + (unsigned)s;
            const int ps = (s - 1) & 1;
            u32x4 fq[SP_NS - 1][2];
#ifdef PV_SPLIT_FENCES
            if (tid == 0) {
#pragma unroll
                for (int k = 1; k < SP_NS; k++) {
                    const int* f = flags_td + ((part + k) % SP_NS) * SP_FLAG_STRIDE;
                    int spins = 0;
                    while ((unsigned)__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != want) {
                        __builtin_amdgcn_s_sleep(1);
                        if (++spins > a.spin_limit) { atomicAdd(a.err, 1); break; }
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < SP_NS - 1; u++)
#pragma unroll
                for (int g = 0; g < 2; g++)
                    fq[u][g] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(hsr, (unsigned)tid * 16u, hx_off(ps, (part + 1 + u) % SP_NS, g), 0));
#else
            int spins = 0;
            while (true) {   // bounded: a lost partner ends in wrong results, never in a hung device
                bool ok = true;
#pragma unroll
                for (int u = 0; u < SP_NS - 1; u++)
#pragma unroll
                    for (int g = 0; g < 2; g++) {
                        fq[u][g] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(hsr, (unsigned)tid * 16u, hx_off(ps, (part + 1 + u) % SP_NS, g), SP_SC1));
                        ok = ok && fq[u][g][1] == want && fq[u][g][3] == want;
                    }
                asm volatile("" ::: "memory");   // the loads are repeated, not hoisted
                if (ok) break;
                if (++spins > a.spin_limit) { atomicAdd(a.err, 1); break; }
            }
#endif
            float* hc = hbuf + cur * TR * LDH;
#pragma unroll
            for (int u = 0; u < SP_NS - 1; u++) {
                const int fp = (part + 1 + u) % SP_NS;
                float* dst = hc + 4 * ((tid & 63) >> 4) * LDH + UPP * fp + 16 * (tid >> 6) + (tid & 15);
#pragma unroll
                for (int g = 0; g < 2; g++) {
                    // (elements go through scalars: hipcc 7.2 compiles __builtin_bit_cast(float, vec[2]) as element 0)
                    const unsigned lo = fq[u][g][0], hi = fq[u][g][2];
                    dst[(2 * g + 0) * LDH] = __builtin_bit_cast(float, lo);
                    dst[(2 * g + 1) * LDH] = __builtin_bit_cast(float, hi);
                }
            }
        }
        lds_barrier();   // h tile complete; every wave is past its x-part (x_store below overwrites xbuf)
        ring_split<NKB_X, NKB_H, NTOT>(acc, hbuf + cur * TR * LDH, LDH, wr, bq, lane);   // h-part (h_0 = 0: zeros at s = 0)
        // ---- cell update (gate order i,f,g,o) ---------------------------------------------------------------------
        float* hn = hbuf + nxt * TR * LDH;
        float hv[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float ig = sigmoidf_(acc[0][i]);
            const float fg = sigmoidf_(acc[1][i]);
            const float gg = tanhf_fma_(acc[2][i]);
            const float og = sigmoidf_(acc[3][i]);
            const float c = lstm_c_(fg, cst[i], ig, gg);
            cst[i] = c;
            hv[i] = og * tanhf_fma_(c);
        }
        if (s + 1 < T_STEPS) {   // the exchange first: it is what the partners wait for
            const unsigned tag = flag_base + (unsigned)s + 1u;
            // 8-byte stores, one per pair: a 16-byte buffer store with an SGPR soffset has a data hazard on gfx950 that hipcc
            // (ROCm 7.2) does not pad (see k_gemm_bf16x3, rnn_gemm.hip), and an inline-asm store would hide an entry of the vmcnt queue from
            // the compiler's counted waits on the weight ring
#pragma unroll
            for (int i = 0; i < 4; i++) {
                typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
                const u32x2 pr = {__builtin_bit_cast(unsigned, hv[i]), tag};
                __builtin_amdgcn_raw_buffer_store_b64(pr, hsr, (unsigned)tid * 16u + 8u * (i & 1), hx_off(cur, part, i >> 1), SP_SC1);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            (hn + i * LDH)[h_l] = hv[i];
            PV_OSTORE(hv[i], osr, og_l, (unsigned)((t * 2 * H + dir * H + i * T_STEPS * 2 * H) * 4));
        }
        if (s + 1 < T_STEPS) x_store();
#ifdef PV_SPLIT_FENCES
        __syncthreads();   // stores have left, LDS tiles (x_{t+1}, own slice of h_t) are complete
        if (s + 1 < T_STEPS && tid == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(flags_td + part * SP_FLAG_STRIDE, (int)(flag_base + (unsigned)s + 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#else
        lds_barrier();     // LDS tiles (x_{t+1}, own slice of h_t) are complete; nothing in flight is waited for
#endif
    }
}

template <int KP> constexpr size_t lds_lstm_split() { return (size_t)(16 * (KP + 4) + 2 * 16 * (H + 4)) * sizeof(float); }
template <int KP, int TR> constexpr size_t lds_lstm() { return (size_t)(TR * (KP + 4) + 2 * TR * (H + 4)) * sizeof(float); }

static_assert(PV_LSTM_HX_BYTES == (size_t)PV_SP_MAX_TILES * 2 * SP_HX_QUADS * sizeof(u32x4), "exchange buffer size (rnn_f32.hpp)");
static_assert(PV_LSTM_FLAGS_BYTES == (size_t)PV_SP_MAX_TILES * 2 * 4 * SP_FLAG_STRIDE * sizeof(int), "exchange counters size (rnn_f32.hpp)");

}  // namespace

int pv_lstm_f32_prepare() {
    // opt in to > 64 KB of dynamic LDS (exact sizes; static LDS counts against the 160 KB too)
    PV_HIP(hipFuncSetAttribute((const void*)k_lstm_layer<32, true, 32>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_lstm<32, 32>()));
    PV_HIP(hipFuncSetAttribute((const void*)k_lstm_layer<32, true, 16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_lstm<32, 16>()));
    PV_HIP(hipFuncSetAttribute((const void*)k_lstm_layer<512, false, 32>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_lstm<512, 32>()));
    PV_HIP(hipFuncSetAttribute((const void*)k_lstm_layer<512, false, 16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_lstm<512, 16>()));
    PV_HIP(hipFuncSetAttribute((const void*)k_lstm_split<32, true, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_lstm_split<32>()));
    PV_HIP(hipFuncSetAttribute((const void*)k_lstm_split<512, false, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_lstm_split<512>()));
    PV_HIP(hipFuncSetAttribute((const void*)k_lstm_split<32, true, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_lstm_split<32>()));
    PV_HIP(hipFuncSetAttribute((const void*)k_lstm_split<512, false, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_lstm_split<512>()));
    return PV_OK;
}

int pv_lstm_f32_async(pv_ctx* ctx, const pv_lstm_desc& d, hipStream_t st) {
    const bool enc = d.x_i8 != nullptr;
    if (d.form == PV_LSTM_SPLIT4 || d.form == PV_LSTM_SPLIT2) {
        const int sp_ns = d.form == PV_LSTM_SPLIT4 ? 4 : 2, n_t16 = d.n_tiles * 2;
        const unsigned split_grid = (unsigned)(((n_t16 + 3) / 4) * 8 * sp_ns);
        LstmSplitArgs s;
        s.x_i8 = d.x_i8; s.x_f32 = d.x_f32; s.wp = d.wp; s.bias = d.bias; s.out = d.out;
        s.hx = static_cast<u32x4*>(d.hx); s.flags = d.flags; s.B = d.B; s.n_tiles = n_t16; s.epoch = d.epoch; s.layer = enc ? 0 : 1;
        s.err = d.err; s.spin_limit = 1 << ctx->opt.exchange_spin_log2; s.drop_part = ctx->opt.debug_drop_part;
        pv_prof_scope ps(ctx, enc ? "k_lstm_split_enc" : "k_lstm_split_dec", st);
        if (enc) {
            if (sp_ns == 4) k_lstm_split<32, true, 4><<<split_grid, 256, lds_lstm_split<32>(), st>>>(s);
            else k_lstm_split<32, true, 2><<<split_grid, 512, lds_lstm_split<32>(), st>>>(s);
        } else {
            if (sp_ns == 4) k_lstm_split<512, false, 4><<<split_grid, 256, lds_lstm_split<512>(), st>>>(s);
            else k_lstm_split<512, false, 2><<<split_grid, 512, lds_lstm_split<512>(), st>>>(s);
        }
    } else {
        const int tr = d.form == PV_LSTM_ROWS32 ? 32 : 16;
        const int n_lt = d.n_tiles * (ROWS / tr);             // whole 32-row tiles are covered in either form
        const unsigned lstm_grid = (unsigned)(((n_lt + 3) / 4) * 8);
        LstmArgs a;
        a.x_i8 = d.x_i8; a.x_f32 = d.x_f32; a.wp = d.wp; a.bias = d.bias; a.out = d.out; a.B = d.B; a.n_tiles = n_lt;
        pv_prof_scope ps(ctx, enc ? "k_lstm_layer_enc" : "k_lstm_layer_dec", st);
        if (enc) {
            if (tr == 32) k_lstm_layer<32, true, 32><<<lstm_grid, 512, lds_lstm<32, 32>(), st>>>(a);
            else k_lstm_layer<32, true, 16><<<lstm_grid, 512, lds_lstm<32, 16>(), st>>>(a);
        } else {
            if (tr == 32) k_lstm_layer<512, false, 32><<<lstm_grid, 512, lds_lstm<512, 32>(), st>>>(a);
            else k_lstm_layer<512, false, 16><<<lstm_grid, 512, lds_lstm<512, 16>(), st>>>(a);
        }
    }
    return PV_OK;
}
