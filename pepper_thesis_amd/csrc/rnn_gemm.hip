// rnn_gemm.hip — the two GEMMs of the recurrent networks on the bf16 MFMA of gfx950 (MI355X), fp32 accumulation.
//
//   k_gemm_bf16x3          3-term split products of "split8" operands: the decoder input projections and linear_1 of
//        PV_DTYPE_BF16_INPUT_GEMM (P1: rnn_p1.hip; P2: rnn_rec_bf16.hip)
//   k_gemm_bf16x6          6-term products of three-piece operands: the same two products of the split-6 chain of PV_DTYPE_F32
//   k_gemm_x6_stream       the same 6-term product, bit for bit, at K = 512 (the split-6 decoder projection): 48-row A tiles resident
//        in LDS as bf16 pieces, W streamed from L2 in the order of pack_gemm6_stream, no barrier inside an item
// The recurrent layers between them are k_rec_bf16 (rnn_rec_bf16.hip). Operand formats: split8_rows (rnn_pack_host.hpp) and
// split3_planes (split3_host.hpp); both are made on the host, once, and uploaded here (pv_upload_split8, pv_upload_split3).
#include "pv_common.hpp"
#include "mfma_tiles.hpp"
#include "rnn_bf16.hpp"
#include "rnn_pack_host.hpp"

#include <algorithm>
#include <mutex>

namespace {

using namespace pvdev;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// ---- PV_DTYPE_BF16_INPUT_GEMM: the non-recurrent products on the bf16 MFMA with a 3-term split ------------------
// x = x_hi + x_lo, w = w_hi + w_lo (bf16 each); x.w ~= x_hi.w_hi + x_hi.w_lo + x_lo.w_hi, accumulated in fp32: relative
// error ~2^-17 per term (the dropped lo.lo term), i.e. fp32-class results (softmax error ~7e-6 measured) at 3/16 of the
// f32-MFMA cost. Plain bf16 operands miss the 1e-4 bar (3.5e-3). Used for the decoder input projection
// G[b,t,:] = W_ih . enc_out[b,t,:] + b (both directions, N = 2048, K = 512) and for linear_1 (N = 512, K = 16896);
// the recurrent h-part, the cell update and linear_2..5 stay fp32.
struct GemmArgs {
    const unsigned char* A;  // activations, split8 rows of K*4 bytes, [M][K] (k_gemm_bf16x6: fp32 rows)
    const unsigned char* W;  // weights, split8 rows, [N][K] (k_gemm_bf16x6: three bf16 planes [3][N][K], split3_host.hpp)
    const float* bias;    // [N] or NULL
    float* C;             // [splits][M][N] row-major, or (c_quads) [M/4][N][4]: four consecutive rows of a column adjacent
    int64_t M;
    int N, K, splits;
    int tiles_m, tiles_n; // 256 x 256 output tiles (k_gemm_bf16x6: 256 x 128)
    int items;            // tiles_m * tiles_n * splits work items, walked by persistent workgroups
    int c_quads;
    const unsigned* iota; // [1024] = 0 .. 1023: the source of the completion-flag transfers (below)
};

// C = A . W^T (+ bias) with 3-term split-bf16 products (a_hi.w_hi + a_hi.w_lo + a_lo.w_hi) on v_mfma_f32_16x16x32_bf16 (until late in
// round 3: 32x32x16 - same cycles per K step, but the chip sustains more on the 16x16x32 shape and the chain runs 1.4 % faster).
// Persistent workgroups (one per CU, 8 waves as 2 x 4, 128 x 64 outputs per wave = 32 accumulator tiles of 16 x 16) walk
// 256 x 256 output tiles; K in steps of 32. Per K step a workgroup moves 64 KB ({A,W} x {hi,lo} x 256 rows x 64 B) from
// L2/HBM straight into LDS with 64 LDS-DMA wave-instructions (buffer_load_dwordx4 ... lds, 8 per wave, no registers, no
// ds_write): the transfers of step k+1 run during step k's MFMAs into the other half of a double-buffered image. An LDS-DMA
// lands lane-linear (wave base + 16 B per lane), so the XOR swizzle that makes the fragment ds_read_b128 conflict-free
// (16-byte chunk index ^ ((row >> 2) & 3) inside each 64-byte row) is applied on the SOURCE address of every lane. One
// barrier per K step; per step and wave 24 ds_read_b128 feed 96 MFMAs of 16 cycles. Work items are ordered n-tile fastest and dealt to the
// XCDs in groups of one XCD's workgroups, so the CUs of an XCD work on the same few A row tiles at the same time. The K steps
// of a workgroup form ONE stream across its items: the first K step of the next item is requested during the last K step of
// this one like any other (buffer = step parity), so an item ends with its 32 dwordx4 stores per wave (quad layout) and the
// next one's operands are there when they are done; item coordinates advance by a constant step (no division per item).
// (Before: coordinates by division, resources, ten LDS-DMA issues and a barrier BETWEEN two items: 4.6 k + 1.1 k of the
// 13.9 k cycles an item boundary cost, the stores 5.1 k: -DPV_GEMM_STAMPS.)
#ifdef PV_GEMM_STAMPS
// diagnostic build: cycle sums of the K loop's phases (workgroup 0, every wave adds): {wait for the transfers, barrier, MFMA block,
// epilogue + next tile's set-up}, and the K steps counted; read by pv_debug_gemm_stamps
__device__ unsigned long long g_gemm_stamps[8];
#define GSTAMP(i) { unsigned long long now_; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(now_) :: "memory"); gs_acc[i] += now_ - gs_last; gs_last = now_; }
#else
#define GSTAMP(i)
#endif
// (gemm6_body below repeats the item walk, the flag completion, the bias transfer and both epilogues for its own tile shape: a fix
// to that machinery belongs in both)
__device__ __forceinline__ void gemm_body(const GemmArgs& g) {
    constexpr int BM = PV_GEMM_TILE, BN = PV_GEMM_TILE, BK = 32;
    constexpr int ARR = BM * BK * 2;          // bytes of one bf16 operand image (16 KB); buffer = [A_hi | A_lo | W_hi | W_lo]
    extern __shared__ __attribute__((aligned(16))) unsigned char smg[];
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wv >> 2, wc = wv & 3;
    // DMA role: piece p (0, 1) of this wave covers rows 16 * (8p + wv) .. + 15 of an operand image; lane -> row lane >> 2,
    // destination chunk lane & 3, source chunk (lane & 3) ^ ((lane >> 4) & 3) (= ((row >> 2) & 3) swizzle)
    const int d_row = lane >> 2;
    const unsigned d_chunk = (unsigned)((lane & 3) ^ ((lane >> 4) & 3));
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, per_xcd = gridDim.x >> 3;
    const int kslice = g.K / g.splits, nk = kslice / BK;
    const unsigned row_bytes = (unsigned)g.K * 4u;

    // An item's operands: buffer resources of its A row tile / W row tile (+ K slice) and the lane offsets of this wave's pieces.
    // TWO sets: the item being multiplied and the one after it, whose first K step is requested during the last K step of this one.
    struct Item { __amdgpu_buffer_rsrc_t ra, rw; unsigned la[2], lw[2]; int mt, nt, sp; };
    // items of this workgroup: it0, it0 + grid, it0 + 2 grid, ... (group q of per_xcd consecutive items goes to the XCD class
    // q % 8: it = (xcd + 8 q) per_xcd + slot). Coordinates advance by a constant step: no division per tile.
    const int step_n = (int)gridDim.x % g.tiles_n, step_r = (int)gridDim.x / g.tiles_n;
    auto item_setup = [&](Item& I) {
        const int64_t m0 = (int64_t)I.mt * BM;
        const int n0 = I.nt * BN;
        I.ra = make_rsrc(g.A + ((size_t)m0 * g.K + (size_t)I.sp * kslice) * 4);
        I.rw = make_rsrc(g.W + ((size_t)n0 * g.K + (size_t)I.sp * kslice) * 4);
#pragma unroll
        for (int p = 0; p < 2; p++) {
            int64_t r = 16 * (8 * p + wv) + d_row;
            if (m0 + r >= g.M) r = g.M - 1 - m0;             // rows beyond M replicate the last row (never stored)
            I.la[p] = (unsigned)r * row_bytes + d_chunk * 32u;
            int rn = 16 * (8 * p + wv) + d_row;
            if (n0 + rn >= g.N) rn = g.N - 1 - n0;
            I.lw[p] = (unsigned)rn * row_bytes + d_chunk * 32u;
        }
    };
    // piece j = 0..7 of this wave for K step kt of item I into buffer buf: (p = j >> 2) x {A_hi, A_lo, W_hi, W_lo}
    auto dma_piece = [&](const Item& I, int kt, int buf, int j) {
        typedef __attribute__((address_space(3))) void* lds_ptr;
        unsigned char* base = smg + buf * 4 * ARR + wv * 1024;
        const unsigned so = (unsigned)(kt * BK * 4);
        const int p = j >> 2, arr = j & 3;
#ifdef PV_GEMM_ABL   // timing experiment (wrong results): bit 0 drops the A pieces, bit 1 the W pieces
        if (((PV_GEMM_ABL) & 1) && arr < 2) return;
        if (((PV_GEMM_ABL) & 2) && arr >= 2) return;
#endif
        if (arr < 2) __builtin_amdgcn_raw_ptr_buffer_load_lds(I.ra, (lds_ptr)(base + arr * ARR + p * 8192), 16, I.la[p], so + (arr & 1 ? 16u : 0u), 0, 0);
        else __builtin_amdgcn_raw_ptr_buffer_load_lds(I.rw, (lds_ptr)(base + arr * ARR + p * 8192), 16, I.lw[p], so + (arr & 1 ? 16u : 0u), 0, 0);
    };
    // the bias of an item's 256 columns also arrives by LDS-DMA (one 1 KB piece, wave 0) into one of two slots behind the operand
    // buffers (items alternate: the next item's bias travels while this one's is still to be read): the kernel holds no
    // register-destination load at all (one consumed while LDS-DMAs are in flight makes hipcc drain the whole vmcnt queue there)
    float* sbias = reinterpret_cast<float*>(smg + 2 * 4 * ARR);
    auto dma_bias = [&](int nt_, int bslot) {
        typedef __attribute__((address_space(3))) void* lds_ptr;
        if (g.bias && wv == 0)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(make_rsrc(g.bias + nt_ * BN), (lds_ptr)(sbias + bslot * BN), 16, (unsigned)lane * 16u, 0, 0, 0);
    };
#ifndef PV_GEMM_VMCNT
    // Completion of a K step's transfers WITHOUT s_waitcnt vmcnt: the counter also holds the epilogue stores of the previous
    // tile (256 KB per workgroup). Loads complete in issue order, so behind the pieces of a K step every wave issues one more
    // LDS-DMA that copies the word iota[seq] into its own flag slot, and polls that slot in LDS until the word is there: the
    // pieces before it have landed, whatever the stores are doing.
    unsigned* sflag = reinterpret_cast<unsigned*>(smg + 2 * 4 * ARR + 2048) + wv * 64;   // 256 B per wave
    sflag[lane] = 0xFFFFFFFFu;
    unsigned seq = 0;
    const __amdgpu_buffer_rsrc_t riota = make_rsrc(g.iota);
    auto dma_flag = [&]() {
        typedef __attribute__((address_space(3))) void* lds_ptr;
        seq = (seq + 1u) & 1023u;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(riota, (lds_ptr)sflag, 4, 0u, seq * 4u, 0, 0);
    };
    // (the poll is a ds_read_b32 from inline asm: a C++ load of LDS that may alias an LDS-DMA target makes hipcc wait for
    // vmcnt(0) in front of it - the very wait this replaces - and a volatile one becomes a flat load)
    const unsigned flag_addr = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned*)(sflag + lane);
    auto dma_wait = [&]() {
        while (true) {
            unsigned v;
            asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(flag_addr) : "memory");
            if (__builtin_amdgcn_ballot_w64(v != seq) == 0) break;
            __builtin_amdgcn_s_sleep(1);
        }
    };
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#else
    auto dma_flag = [&]() {};
    auto dma_wait = [&]() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };
#endif
    int it = xcd * per_xcd + slot;
    Item cur, nxt;
    cur.mt = cur.nt = cur.sp = 0;
    int r_cur = 0;                                // it / tiles_n of the current item
    unsigned gstep = 0;                           // K steps of this workgroup so far: step s uses operand buffer s & 1, across items
    int tile_no = 0;                              // items so far: bias slot tile_no & 1
    if (it < g.items) {
        cur.nt = it % g.tiles_n;
        r_cur = it / g.tiles_n;
        cur.sp = r_cur % g.splits;
        cur.mt = r_cur / g.splits;
        item_setup(cur);
#pragma unroll
        for (int j = 0; j < 8; j++) dma_piece(cur, 0, 0, j);
        dma_bias(cur.nt, 0);
        dma_flag();
    }
#ifdef PV_GEMM_STAMPS
    unsigned long long gs_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, gs_last;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(gs_last) :: "memory");
#endif
    while (it < g.items) {
        // the item after this one (its first K step is requested during this item's last)
        const int it_n = it + (int)gridDim.x;
        const bool has_next = it_n < g.items;
        int r_n = r_cur + step_r;
        nxt.nt = cur.nt + step_n;
        if (nxt.nt >= g.tiles_n) { nxt.nt -= g.tiles_n; r_n++; }
        if (g.splits == 1) { nxt.sp = 0; nxt.mt = r_n; }
        else { nxt.sp = r_n % g.splits; nxt.mt = r_n / g.splits; }
        if (has_next) item_setup(nxt);
        GSTAMP(6)
        f32x4 acc[8][4];   // 16 x 16 tiles of this wave's 128 x 64 outputs
#pragma unroll
        for (int mi = 0; mi < 8; mi++)
#pragma unroll
            for (int ni = 0; ni < 4; ni++)
#pragma unroll
                for (int r = 0; r < 4; r++) acc[mi][ni][r] = 0.0f;
        // one K step: wait for its operands, multiply, and request the operands of the step after it - K step s_kt of item S -
        // into the other buffer (issue == false: there is no such step)
        auto k_step = [&](const Item& S, int s_kt, bool issue, bool next_bias) {
            const int buf = (int)(gstep & 1u);
            // this step's operands have landed (every wave waits for its own DMAs, then the barrier); the other buffer is free:
            // every wave is past the step that read it.
            // (a counted wait that lets the previous item's epilogue stores stay in flight is NOT safe here: vmcnt retires loads
            // in order among loads and stores among stores, but a store may retire before an older LDS-DMA load, so "at most 32
            // outstanding" does not imply the DMAs have landed. It gave a sporadic 1e-4 error in one of five full test runs.)
            GSTAMP(3)
            dma_wait();
            GSTAMP(0)
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            GSTAMP(1)
            const unsigned char* base = smg + buf * 4 * ARR;
            // the next step's eight pieces are issued between the blocks of this step's MFMAs instead of as a burst behind the
            // barrier: an LDS-DMA costs its wave ~100-150 issue cycles, and the two waves of a SIMD - phase-locked by the barrier
            // - both paid the eight of them before either issued an MFMA (~1200 of a K step's ~4300 cycles). Two per block in the
            // FIRST half of the step: one per block over the whole step left the last pieces ~400 cycles to land before the step
            // ended (the step then waited ~650 cycles for them); four or eight in front of the first blocks stall the pipe again
            // (decoder projection, same box: 1.49 ms one per block, 1.43 two, 1.48 four, 1.46 eight).
            // v_mfma_f32_16x16x32_bf16: a K step is ONE k-step of 32; lane -> row / column lane & 15, 16-byte chunk lane >> 4 of the
            // 64-byte row (under the image's XOR swizzle: conflict-free as the 32 x 32 x 16 reads were). Same MFMA cycles and LDS
            // reads per K step as the 32 x 32 x 16 form, but the chip sustains ~14 % more FLOP/s on this shape under load
            // (tools/dbg/src/mfma_shapes.hip: 2.42 against 2.12 PFLOP/s in a bare loop - the kernel runs power-limited at
            // ~1.8 GHz).
            {
                const unsigned ch16 = (unsigned)((((lane >> 4)) ^ (((lane & 15) >> 2) & 3)) * 16);
                const unsigned fa16 = (unsigned)((128 * wr + (lane & 15)) * 64), fb16 = (unsigned)(2 * ARR + (64 * wc + (lane & 15)) * 64);
                bf16x8 bp[2][4];   // {hi, lo} pieces
#pragma unroll
                for (int ni = 0; ni < 4; ni++) {
                    bp[0][ni] = *reinterpret_cast<const bf16x8*>(base + fb16 + ni * 16 * 64 + ch16);
                    bp[1][ni] = *reinterpret_cast<const bf16x8*>(base + ARR + fb16 + ni * 16 * 64 + ch16);
                }
#pragma unroll
                for (int mi = 0; mi < 8; mi++) {
                    bf16x8 ap[2];
                    ap[0] = *reinterpret_cast<const bf16x8*>(base + fa16 + mi * 16 * 64 + ch16);
                    ap[1] = *reinterpret_cast<const bf16x8*>(base + ARR + fa16 + mi * 16 * 64 + ch16);
                    if (issue && mi < 4) {   // two pieces in front of each of the first four blocks
                        dma_piece(S, s_kt, buf ^ 1, 2 * mi);
                        dma_piece(S, s_kt, buf ^ 1, 2 * mi + 1);
                        if (mi == 3) {
                            if (next_bias) dma_bias(nxt.nt, (tile_no + 1) & 1);
                            dma_flag();
                        }
                    }
#pragma unroll
                    for (int ni = 0; ni < 4; ni++) {
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ap[0], bp[0][ni], acc[mi][ni], 0, 0, 0);
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ap[0], bp[1][ni], acc[mi][ni], 0, 0, 0);
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ap[1], bp[0][ni], acc[mi][ni], 0, 0, 0);
                    }
                }
            }
            GSTAMP(2)
#ifdef PV_GEMM_STAMPS
            gs_acc[4]++;
#endif
            gstep++;
        };
        for (int kt = 0; kt + 1 < nk; kt++) k_step(cur, kt + 1, true, false);
        k_step(nxt, 0, has_next, true);          // the last step requests step 0 of the next item (and its bias)
        // C tile as a sized buffer resource: rows beyond M fall outside it and are dropped by the bounds check; the
        // address of every store is (tile resource) + (lane offset) + (scalar offset of (wave, mi, ni, r))
        const int64_t m0 = (int64_t)cur.mt * BM;
        const int n0 = cur.nt * BN;
        const int64_t rows_left = g.M - m0 < BM ? g.M - m0 : BM;
        float* cbase = g.C + (size_t)cur.sp * g.M * g.N;
        float bv[4];
        // (this item's bias slot is written again during the last K step of the NEXT item: every wave has read it long before)
#pragma unroll
        for (int ni = 0; ni < 4; ni++) bv[ni] = g.bias ? sbias[(tile_no & 1) * BN + 64 * wc + 16 * ni + (lane & 15)] : 0.0f;
        GSTAMP(5)
        if (g.c_quads) {
            // [M/4][N][4]: the four registers of a 16 x 16 accumulator are four consecutive rows of one column: one 16-byte store,
            // lane -> quad row lane >> 4, column lane & 15
            const uint64_t cptr = (uint64_t)(cbase + ((size_t)(m0 >> 2) * g.N + n0) * 4);
            u32x4 rcw;
            rcw[0] = __builtin_amdgcn_readfirstlane((unsigned)cptr);
            rcw[1] = __builtin_amdgcn_readfirstlane((unsigned)(cptr >> 32) & 0xffffu);
            rcw[2] = __builtin_amdgcn_readfirstlane((unsigned)((((rows_left + 3) / 4 - 1) * g.N + BN) * 16));
            rcw[3] = 0x00020000u;
            const unsigned c_l = (unsigned)((((lane >> 4)) * g.N + (lane & 15)) * 16);
#pragma unroll
            for (int mi = 0; mi < 8; mi++)
#pragma unroll
                for (int ni = 0; ni < 4; ni++) {
                    f32x4 v;
#pragma unroll
                    for (int j = 0; j < 4; j++) v[j] = acc[mi][ni][j] + bv[ni];
                    // (inline asm with its own wait states: see the 32 x 32 form's note on gfx950's late read of store data)
                    const unsigned so = (unsigned)(((32 * wr + 4 * mi) * g.N + 64 * wc + 16 * ni) * 16);
                    asm volatile("s_nop 4\n\tbuffer_store_dwordx4 %0, %1, %2, %3 offen nt\n\ts_nop 2"
                                 :: "v"(v), "v"(c_l), "s"(rcw), "s"(so) : "memory");
                }
        } else {
            const __amdgpu_buffer_rsrc_t rc = make_rsrc_sized(cbase + (size_t)m0 * g.N + n0, (unsigned)(((rows_left - 1) * g.N + BN) * 4));
            const unsigned c_l = (unsigned)(((4 * (lane >> 4)) * g.N + (lane & 15)) * 4);
#pragma unroll
            for (int mi = 0; mi < 8; mi++)
#pragma unroll
                for (int ni = 0; ni < 4; ni++)
#pragma unroll
                    for (int r = 0; r < 4; r++)
                        buf_store1_nt(acc[mi][ni][r] + bv[ni], rc, c_l, (unsigned)(((128 * wr + 16 * mi + r) * g.N + 64 * wc + 16 * ni) * 4));
        }
        GSTAMP(7)
        cur = nxt;
        r_cur = r_n;
        it = it_n;
        tile_no++;
    }
#ifdef PV_GEMM_STAMPS
    if (blockIdx.x == 0 && lane == 0)
        for (int i = 0; i < 8; i++) atomicAdd(&g_gemm_stamps[i], gs_acc[i]);
#endif
}

// ---- k_gemm_bf16x6 (PV_DTYPE_F32 split-6 chain): six-term products of three-piece operands ------------------------------
// x = x0 + x1 + x2 (bf16 each, split3_bf16 / split3_host.hpp); x.w = a2.b0 + a0.b2 + a1.b1 + a0.b0 + a0.b1 + a1.b0 in that
// order, the small terms first (the dropped a1.b2, a2.b1, a2.b2 are below 2^-24 relative). A is the fp32 output of the layer
// before, rows [M][K]; W is the model's weights, which do not change between load and close: they are split ONCE, on the
// host, into three bf16 planes [3][N][K] (split3_planes), and only A is split in the kernel - by the one wave that owns the rows.
// A work item is 256 (M) x 128 (N); the waves go 8 x 1: wave w owns rows 32 w .. 32 w + 31 and all 128 columns (2 x 8 accumulator
// tiles). Per K step of 32 a workgroup moves
//     A   256 rows x 128 B of fp32 as the "hi" image (elements 0..3 of every 8-group) and the "lo" image (4..7), 2 x 16 KB: an
//         fp32 8-group is 32 bytes like a split8 group, so these transfers are byte for byte those of the 3-term form
//     W   three piece images of 128 rows x 64 B, 3 x 8 KB, row pitch K * 2
// = 56 KB per stage, 112 KB double-buffered, in 16-row x 64 B LDS-DMA pieces with the XOR swizzle of the 3-term form on the
// source address: 7 pieces per wave and stage (4 of A, one of each W plane). A wave reads its two A fragments as fp32 and
// splits them (no other wave touches those rows), holds the six pieces, and streams the 8 x 3 W fragments over ni straight as
// bf16x8: ~90 VALU instructions beside 96 MFMAs per step (256 x 256 items with all eight waves splitting 8 + 4 fragments:
// ~530 beside 192, issue-bound; 256 x 256 with W piece images would need 160 KB for the operands alone). Everything else is
// the 3-term form's machinery (above): the persistent item walk, n-tile fastest, dealt to the XCDs in groups; one K-step
// stream across items; completion by flag transfer; bias by LDS-DMA; the next step's pieces issued between the first MFMA
// blocks of this one; both epilogues. That machinery is repeated here from gemm_body, not shared: a fix to it belongs in both.
constexpr int PV_GEMM6_BN = 128;   // columns of one work item of k_gemm_bf16x6 (a kernel and launcher detail: the plan counts 256 x 256 tiles)
__device__ __forceinline__ void gemm6_body(const GemmArgs& g) {
    constexpr int BM = PV_GEMM_TILE, BN = PV_GEMM6_BN, BK = 32;
    constexpr int ARR = BM * BK * 2;          // bytes of one A image (16 KB)
    constexpr int WRR = BN * BK * 2;          // bytes of one W piece image (8 KB)
    constexpr int STAGE = 2 * ARR + 3 * WRR;  // [A_hi | A_lo | W_0 | W_1 | W_2]
    extern __shared__ __attribute__((aligned(16))) unsigned char smg[];
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    // DMA role: this wave moves rows 16 * (8p + wv) .. + 15 (p = 0, 1) of both A images and rows 16 * wv .. + 15 of every W piece
    // image; lane -> row lane >> 2, destination chunk lane & 3, source chunk (lane & 3) ^ ((lane >> 4) & 3)
    const int d_row = lane >> 2;
    const unsigned d_chunk = (unsigned)((lane & 3) ^ ((lane >> 4) & 3));
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, per_xcd = gridDim.x >> 3;
    const int kslice = g.K / g.splits, nk = kslice / BK;
    const unsigned a_pitch = (unsigned)g.K * 4u, w_pitch = (unsigned)g.K * 2u;
    const unsigned plane_bytes = (unsigned)g.N * w_pitch;

    struct Item { __amdgpu_buffer_rsrc_t ra, rw; unsigned la[2], lw; int mt, nt, sp; };
    const int step_n = (int)gridDim.x % g.tiles_n, step_r = (int)gridDim.x / g.tiles_n;
    auto item_setup = [&](Item& I) {
        const int64_t m0 = (int64_t)I.mt * BM;
        const int n0 = I.nt * BN;
        I.ra = make_rsrc(g.A + ((size_t)m0 * g.K + (size_t)I.sp * kslice) * 4);
        I.rw = make_rsrc(g.W + ((size_t)n0 * g.K + (size_t)I.sp * kslice) * 2);
#pragma unroll
        for (int p = 0; p < 2; p++) {
            int64_t r = 16 * (8 * p + wv) + d_row;
            if (m0 + r >= g.M) r = g.M - 1 - m0;             // rows beyond M replicate the last row (never stored)
            I.la[p] = (unsigned)r * a_pitch + d_chunk * 32u;
        }
        I.lw = (unsigned)(16 * wv + d_row) * w_pitch + d_chunk * 16u;   // (N is a multiple of the item's 128 columns)
    };
    // piece j = 0..6 of this wave for K step kt of item I into buffer buf: j < 4: (p = j >> 1) x {A_hi, A_lo}; j >= 4: W plane j - 4
    auto dma_piece = [&](const Item& I, int kt, int buf, int j) {
        typedef __attribute__((address_space(3))) void* lds_ptr;
        unsigned char* base = smg + buf * STAGE + wv * 1024;
        if (j < 4) {
            const int p = j >> 1, arr = j & 1;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(I.ra, (lds_ptr)(base + arr * ARR + p * 8192), 16, I.la[p], (unsigned)(kt * BK * 4) + (arr ? 16u : 0u), 0, 0);
        } else {
            const int q = j - 4;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(I.rw, (lds_ptr)(base + 2 * ARR + q * WRR), 16, I.lw, (unsigned)(kt * BK * 2) + (unsigned)q * plane_bytes, 0, 0);
        }
    };
    // the bias of an item's 128 columns by LDS-DMA (waves 0 and 1, 64 floats each) into one of two slots behind the operand buffers
    float* sbias = reinterpret_cast<float*>(smg + 2 * STAGE);
    auto dma_bias = [&](int nt_, int bslot) {
        typedef __attribute__((address_space(3))) void* lds_ptr;
        if (g.bias && wv < 2)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(make_rsrc(g.bias + nt_ * BN + wv * 64), (lds_ptr)(sbias + bslot * BN + wv * 64), 4, (unsigned)lane * 4u, 0, 0, 0);
    };
    // completion of a K step's transfers by flag transfer, as in the 3-term form
    unsigned* sflag = reinterpret_cast<unsigned*>(smg + 2 * STAGE + 2048) + wv * 64;   // 256 B per wave
    sflag[lane] = 0xFFFFFFFFu;
    unsigned seq = 0;
    const __amdgpu_buffer_rsrc_t riota = make_rsrc(g.iota);
    auto dma_flag = [&]() {
        typedef __attribute__((address_space(3))) void* lds_ptr;
        seq = (seq + 1u) & 1023u;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(riota, (lds_ptr)sflag, 4, 0u, seq * 4u, 0, 0);
    };
    const unsigned flag_addr = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned*)(sflag + lane);
    auto dma_wait = [&]() {
        while (true) {
            unsigned v;
            asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(flag_addr) : "memory");
            if (__builtin_amdgcn_ballot_w64(v != seq) == 0) break;
            __builtin_amdgcn_s_sleep(1);
        }
    };
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    int it = xcd * per_xcd + slot;
    Item cur, nxt;
    cur.mt = cur.nt = cur.sp = 0;
    int r_cur = 0;                                // it / tiles_n of the current item
    unsigned gstep = 0;                           // K steps of this workgroup so far: step s uses operand buffer s & 1, across items
    int tile_no = 0;                              // items so far: bias slot tile_no & 1
    if (it < g.items) {
        cur.nt = it % g.tiles_n;
        r_cur = it / g.tiles_n;
        cur.sp = r_cur % g.splits;
        cur.mt = r_cur / g.splits;
        item_setup(cur);
#pragma unroll
        for (int j = 0; j < 7; j++) dma_piece(cur, 0, 0, j);
        dma_bias(cur.nt, 0);
        dma_flag();
    }
#ifdef PV_GEMM_STAMPS
    unsigned long long gs_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, gs_last;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(gs_last) :: "memory");
#endif
    while (it < g.items) {
        const int it_n = it + (int)gridDim.x;
        const bool has_next = it_n < g.items;
        int r_n = r_cur + step_r;
        nxt.nt = cur.nt + step_n;
        if (nxt.nt >= g.tiles_n) { nxt.nt -= g.tiles_n; r_n++; }
        if (g.splits == 1) { nxt.sp = 0; nxt.mt = r_n; }
        else { nxt.sp = r_n % g.splits; nxt.mt = r_n / g.splits; }
        if (has_next) item_setup(nxt);
        GSTAMP(6)
        f32x4 acc[2][8];   // 16 x 16 tiles of this wave's 32 x 128 outputs
#pragma unroll
        for (int mi = 0; mi < 2; mi++)
#pragma unroll
            for (int ni = 0; ni < 8; ni++)
#pragma unroll
                for (int r = 0; r < 4; r++) acc[mi][ni][r] = 0.0f;
        auto k_step = [&](const Item& S, int s_kt, bool issue, bool next_bias) {
            const int buf = (int)(gstep & 1u);
            GSTAMP(3)
            dma_wait();
            GSTAMP(0)
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            GSTAMP(1)
            const unsigned char* base = smg + buf * STAGE;
            // lane -> row / column lane & 15, 16-byte chunk lane >> 4 of the 64-byte image row (under the XOR swizzle)
            const unsigned ch16 = (unsigned)((((lane >> 4)) ^ (((lane & 15) >> 2) & 3)) * 16);
            const unsigned fa16 = (unsigned)((32 * wv + (lane & 15)) * 64) + ch16, fb16 = (unsigned)(2 * ARR + (lane & 15) * 64) + ch16;
            bf16x8 ap[2][3];   // this wave's A pieces of the step: split here, by no other wave
#pragma unroll
            for (int mi = 0; mi < 2; mi++)
                split3_bf16(*reinterpret_cast<const f32x4*>(base + fa16 + mi * 16 * 64),
                            *reinterpret_cast<const f32x4*>(base + ARR + fa16 + mi * 16 * 64), ap[mi][0], ap[mi][1], ap[mi][2]);
#pragma unroll
            for (int ni = 0; ni < 8; ni++) {
                bf16x8 bp[3];
#pragma unroll
                for (int q = 0; q < 3; q++) bp[q] = *reinterpret_cast<const bf16x8*>(base + fb16 + q * WRR + ni * 16 * 64);
                // the next step's seven pieces go out in front of the first four blocks (two each), the flag transfer behind them
                if (issue && ni < 4) {
                    dma_piece(S, s_kt, buf ^ 1, 2 * ni);
                    if (ni < 3) dma_piece(S, s_kt, buf ^ 1, 2 * ni + 1);
                    else {
                        if (next_bias) dma_bias(nxt.nt, (tile_no + 1) & 1);
                        dma_flag();
                    }
                }
                // per output element the six terms in the order above; the two row tiles alternate, so that consecutive MFMAs
                // do not depend on each other
#pragma unroll
                for (int mi = 0; mi < 2; mi++) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ap[mi][2], bp[0], acc[mi][ni], 0, 0, 0);
#pragma unroll
                for (int mi = 0; mi < 2; mi++) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ap[mi][0], bp[2], acc[mi][ni], 0, 0, 0);
#pragma unroll
                for (int mi = 0; mi < 2; mi++) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ap[mi][1], bp[1], acc[mi][ni], 0, 0, 0);
#pragma unroll
                for (int mi = 0; mi < 2; mi++) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ap[mi][0], bp[0], acc[mi][ni], 0, 0, 0);
#pragma unroll
                for (int mi = 0; mi < 2; mi++) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ap[mi][0], bp[1], acc[mi][ni], 0, 0, 0);
#pragma unroll
                for (int mi = 0; mi < 2; mi++) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ap[mi][1], bp[0], acc[mi][ni], 0, 0, 0);
            }
            GSTAMP(2)
#ifdef PV_GEMM_STAMPS
            gs_acc[4]++;
#endif
            gstep++;
        };
        for (int kt = 0; kt + 1 < nk; kt++) k_step(cur, kt + 1, true, false);
        k_step(nxt, 0, has_next, true);          // the last step requests step 0 of the next item (and its bias)
        // C tile as a sized buffer resource: rows beyond M fall outside it and are dropped by the bounds check
        const int64_t m0 = (int64_t)cur.mt * BM;
        const int n0 = cur.nt * BN;
        const int64_t rows_left = g.M - m0 < BM ? g.M - m0 : BM;
        float* cbase = g.C + (size_t)cur.sp * g.M * g.N;
        float bv[8];
#pragma unroll
        for (int ni = 0; ni < 8; ni++) bv[ni] = g.bias ? sbias[(tile_no & 1) * BN + 16 * ni + (lane & 15)] : 0.0f;
        GSTAMP(5)
        if (g.c_quads) {
            // [M/4][N][4]: one 16-byte store per accumulator tile, lane -> quad row lane >> 4, column lane & 15
            const uint64_t cptr = (uint64_t)(cbase + ((size_t)(m0 >> 2) * g.N + n0) * 4);
            u32x4 rcw;
            rcw[0] = __builtin_amdgcn_readfirstlane((unsigned)cptr);
            rcw[1] = __builtin_amdgcn_readfirstlane((unsigned)(cptr >> 32) & 0xffffu);
            rcw[2] = __builtin_amdgcn_readfirstlane((unsigned)((((rows_left + 3) / 4 - 1) * g.N + BN) * 16));
            rcw[3] = 0x00020000u;
            const unsigned c_l = (unsigned)((((lane >> 4)) * g.N + (lane & 15)) * 16);
#pragma unroll
            for (int mi = 0; mi < 2; mi++)
#pragma unroll
                for (int ni = 0; ni < 8; ni++) {
                    f32x4 v;
#pragma unroll
                    for (int j = 0; j < 4; j++) v[j] = acc[mi][ni][j] + bv[ni];
                    const unsigned so = (unsigned)(((8 * wv + 4 * mi) * g.N + 16 * ni) * 16);
                    asm volatile("s_nop 4\n\tbuffer_store_dwordx4 %0, %1, %2, %3 offen nt\n\ts_nop 2"
                                 :: "v"(v), "v"(c_l), "s"(rcw), "s"(so) : "memory");
                }
        } else {
            const __amdgpu_buffer_rsrc_t rc = make_rsrc_sized(cbase + (size_t)m0 * g.N + n0, (unsigned)(((rows_left - 1) * g.N + BN) * 4));
            const unsigned c_l = (unsigned)(((4 * (lane >> 4)) * g.N + (lane & 15)) * 4);
#pragma unroll
            for (int mi = 0; mi < 2; mi++)
#pragma unroll
                for (int ni = 0; ni < 8; ni++)
#pragma unroll
                    for (int r = 0; r < 4; r++)
                        buf_store1_nt(acc[mi][ni][r] + bv[ni], rc, c_l, (unsigned)(((32 * wv + 16 * mi + r) * g.N + 16 * ni) * 4));
        }
        GSTAMP(7)
        cur = nxt;
        r_cur = r_n;
        it = it_n;
        tile_no++;
    }
#ifdef PV_GEMM_STAMPS
    if (blockIdx.x == 0 && lane == 0)
        for (int i = 0; i < 8; i++) atomicAdd(&g_gemm_stamps[i], gs_acc[i]);
#endif
}

// (two kernels, no template: a __launch_bounds__(512, 2) kernel template loses its host stub in this compiler)
__global__ __launch_bounds__(512, 2) void k_gemm_bf16x3(GemmArgs g) { gemm_body(g); }
__global__ __launch_bounds__(512, 2) void k_gemm_bf16x6(GemmArgs g) { gemm6_body(g); }

// ---- k_gemm_x6_stream: the six-term product at K = 512 with A resident in LDS and W streamed from L2 --------------------------
// The decoder input projection has K = 512 only: the whole K extent of a 48-row tile fits in LDS as its three bf16 pieces, so the
// product takes the recurrent kernels' structure (ring_x6_16, rnn_rec_bf16.hip) instead of a staged GEMM's. A work item is 48 rows
// x all N columns; persistent workgroups (one per CU, 8 waves) walk the items, and every workgroup reads W in the same order.
//   item prologue   the item's fp32 rows (rows past M read as zeros and are never stored), split ONCE with split3_bf16 by the lane
//                   that loaded them, into three piece planes [48 rows][K] of bf16 in LDS, row pitch 1040 B (260 dwords = 4 mod
//                   64: the bank rule of RecCfg::HS); one barrier in front (every wave is done with the old tile), one behind
//   main loop       no workgroup barrier. Wave w owns columns [w N / 8, (w + 1) N / 8) and walks them in blocks of 64 (four column
//                   tiles), the 16 k-steps inside a block: 3 x 4 accumulator tiles. A fragments: nine ds_read_b128 per k-step,
//                   requested one k-step ahead into a second register set. W fragments: the stream of pack_gemm6_stream through a
//                   ring of GS_D slots (three pieces, 12 registers each) on raw buffer loads GS_D - 1 slots ahead, fenced with
//                   sched_barrier as in ring_x6_16; the ring runs on across blocks and wraps into the next item.
//   MFMA order      v_mfma_f32_16x16x32_bf16, lane group g = k 8g .. 8g + 7 of the step; per accumulator tile the k-steps ascend and
//                   the six terms go a2.b0, a0.b2, a1.b1, a0.b0, a0.b1, a1.b0, the three row tiles alternating: per output element
//                   the sequence of gemm6_body, so C is bit-identical to k_gemm_bf16x6's
//   epilogue        acc + bias (from LDS, loaded once per launch), every wave's block ends in its own nt stores through a sized
//                   resource that drops rows past M; both layouts
// No flags, no atomics, nothing between workgroups.
constexpr int GS_ROWS = 48, GS_K = 512, GS_PITCH = GS_K * 2 + 16, GS_PLANE = GS_ROWS * GS_PITCH, GS_D = 8;
constexpr int GS_MAXN = 2048;   // columns of the bias image in LDS
constexpr size_t LDS_GEMM_STREAM = (size_t)3 * GS_PLANE + GS_MAXN * 4;   // 149 760 B of pieces + 8 KB of bias
struct GemmStreamArgs {
    const float* A;           // [M][512] fp32 rows
    const unsigned char* Ws;  // pack_gemm6_stream
    const float* bias;        // [N] or NULL
    float* C;                 // [M][N], or (c_quads) [M/4][N][4]
    int64_t M;
    int N, c_quads, items;    // items of 48 rows
};
#ifdef PV_GEMM_STAMPS
#define SSTAMP(i) { unsigned long long now_; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(now_) :: "memory"); gs_acc[i] += now_ - gs_last; gs_last = now_; }
#else
#define SSTAMP(i)
#endif
__global__ __launch_bounds__(512) void k_gemm_x6_stream(GemmStreamArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smg[];
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ncol_w = g.N >> 3, nblk = ncol_w >> 6;          // columns of a wave, blocks of 64 of them
    const __amdgpu_buffer_rsrc_t wr = make_rsrc(g.Ws + (size_t)wv * (size_t)nblk * (64 * 3072));
    const unsigned lane16 = (unsigned)lane * 16u;
    float* sbias = reinterpret_cast<float*>(smg + 3 * GS_PLANE);
    for (int n = tid; n < g.N; n += 512) sbias[n] = g.bias ? g.bias[n] : 0.0f;   // (published by the first item's barriers)
    // the ring: slots 0 .. GS_D - 2 of the wave's stream are on their way when an item starts
    f32x4 bq[GS_D][3];
#pragma unroll
    for (int q = 0; q < GS_D - 1; q++)
#pragma unroll
        for (int p = 0; p < 3; p++) bq[q][p] = buf_load4(wr, lane16, (unsigned)(q * 3072 + p * 1024));
    // A fragments: lane -> row 16 mi + (lane & 15), k-group lane >> 4 of the k-step
    const unsigned char* a_l = smg + (lane & 15) * GS_PITCH + (lane >> 4) * 16;
#ifdef PV_GEMM_STAMPS
    unsigned long long gs_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, gs_last, gs_t0, gs_r0;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(gs_last) :: "memory");
    gs_t0 = gs_last;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(gs_r0) :: "memory");
#endif
    for (int it = blockIdx.x; it < g.items; it += (int)gridDim.x) {
        const int64_t m0 = (int64_t)it * GS_ROWS;
        const int rows_left = (int)(g.M - m0 < GS_ROWS ? g.M - m0 : GS_ROWS);
        // (lane numbers the optimiser cannot see through: what the prologue and the epilogues derive from them is worked out where
        // it is used, a few VALU instructions, and holds no register across the MFMA loop, which has none to spare)
        int lane_p;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane_p));
        {   // item prologue: wave w loads rows w, w + 8, .. w + 40 of the tile, lane -> 8-group lane of the row (32 B of fp32 -> 16 B a piece)
            const unsigned pl_g = (unsigned)wv * (GS_K * 4) + (unsigned)lane_p * 32u;
            unsigned char* pl_s = smg + wv * GS_PITCH + lane_p * 16;
            const __amdgpu_buffer_rsrc_t ra = make_rsrc_sized(g.A + (size_t)m0 * GS_K, (unsigned)rows_left * (GS_K * 4));
            f32x4 raw[6][2];
#pragma unroll
            for (int j = 0; j < 6; j++) {
                raw[j][0] = buf_load4_nt(ra, pl_g, (unsigned)(j * 8 * GS_K * 4));
                raw[j][1] = buf_load4_nt(ra, pl_g, (unsigned)(j * 8 * GS_K * 4 + 16));
            }
            lds_barrier();   // every wave has read the last of the tile before
#pragma unroll
            for (int j = 0; j < 6; j++) {
                bf16x8 x0, x1, x2;
                split3_bf16(raw[j][0], raw[j][1], x0, x1, x2);
                *reinterpret_cast<bf16x8*>(pl_s + j * 8 * GS_PITCH) = x0;
                *reinterpret_cast<bf16x8*>(pl_s + j * 8 * GS_PITCH + GS_PLANE) = x1;
                *reinterpret_cast<bf16x8*>(pl_s + j * 8 * GS_PITCH + 2 * GS_PLANE) = x2;
            }
            lds_barrier();
        }
        SSTAMP(0)
        // C of the item as a sized resource: rows past M fall outside it and are dropped by the bounds check
        const __amdgpu_buffer_rsrc_t rc = g.c_quads
            ? make_rsrc_sized(g.C + (size_t)(m0 >> 2) * g.N * 4, (unsigned)(rows_left >> 2) * (unsigned)g.N * 16u)
            : make_rsrc_sized(g.C + (size_t)m0 * g.N, (unsigned)rows_left * (unsigned)g.N * 4u);
#pragma nounroll
        for (int b = 0; b < nblk; b++) {
            const unsigned sb_cur = (unsigned)b * (64 * 3072), sb_nxt = b + 1 < nblk ? sb_cur + 64 * 3072 : 0u;
            f32x4 acc[3][4];
#pragma unroll
            for (int mi = 0; mi < 3; mi++)
#pragma unroll
                for (int ct = 0; ct < 4; ct++)
#pragma unroll
                    for (int r = 0; r < 4; r++) acc[mi][ct][r] = 0.0f;
            bf16x8 ap[2][3][3];   // [set][piece][row tile]
#define GS_A(set, ks)                                                                                   \
    _Pragma("unroll") for (int q = 0; q < 3; q++)                                                        \
        _Pragma("unroll") for (int mi = 0; mi < 3; mi++)                                                 \
            ap[set][q][mi] = *reinterpret_cast<const bf16x8*>(a_l + q * GS_PLANE + mi * 16 * GS_PITCH + (ks) * 64);
            GS_A(0, 0)
#pragma unroll
            for (int i = 0; i < 64; i++) {
                const int ks = i >> 2, ct = i & 3, as = ks & 1;
                {   // request slot i + GS_D - 1 (beyond the block: of the next block, beyond the item: of the next item)
                    const int t = i + GS_D - 1, rs = t % GS_D;
                    const unsigned so = t < 64 ? sb_cur + (unsigned)(t * 3072) : sb_nxt + (unsigned)((t - 64) * 3072);
#pragma unroll
                    for (int p = 0; p < 3; p++) bq[rs][p] = buf_load4(wr, lane16, so + (unsigned)(p * 1024));
                }
                if (ct == 0 && ks + 1 < 16) { GS_A(as ^ 1, ks + 1) }
                __builtin_amdgcn_sched_barrier(0);   // keep hipcc from sinking the prefetches next to their uses
                {
                    const int rs = i % GS_D;
                    const bf16x8 b0 = __builtin_bit_cast(bf16x8, bq[rs][0]), b1 = __builtin_bit_cast(bf16x8, bq[rs][1]);
                    const bf16x8 b2 = __builtin_bit_cast(bf16x8, bq[rs][2]);
#define GS_TERM(AP, BP)             \
    _Pragma("unroll") for (int mi = 0; mi < 3; mi++) acc[mi][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ap[as][AP][mi], BP, acc[mi][ct], 0, 0, 0);
                    GS_TERM(2, b0)
                    GS_TERM(0, b2)
                    GS_TERM(1, b1)
                    GS_TERM(0, b0)
                    GS_TERM(0, b1)
                    GS_TERM(1, b0)
#undef GS_TERM
                }
                __builtin_amdgcn_sched_barrier(0);
            }
#undef GS_A
            SSTAMP(1)
            int lane_e;
            asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane_e));
            const int col_l = wv * ncol_w + 64 * b + (lane_e & 15);   // + 16 ct: this lane's column
            float bv[4];
#pragma unroll
            for (int ct = 0; ct < 4; ct++) bv[ct] = sbias[col_l + 16 * ct];
            // lane part of a C offset, both layouts: rows 4 (lane >> 4) .. + 3 are N * 16 bytes per lane group, a column 16 or 4 bytes
            const unsigned c_l = (unsigned)((lane_e >> 4) * g.N * 16 + col_l * (g.c_quads ? 16 : 4));
            if (g.c_quads) {
                // [M/4][N][4]: the four registers of an accumulator tile are four consecutive rows of one column: one 16-byte store,
                // lane -> quad row lane >> 4, column lane & 15
#pragma unroll
                for (int mi = 0; mi < 3; mi++)
#pragma unroll
                    for (int ct = 0; ct < 4; ct++) {
                        f32x4 v;
#pragma unroll
                        for (int r = 0; r < 4; r++) v[r] = acc[mi][ct][r] + bv[ct];
                        // gfx950 reads the data of a 16-byte store late: the wait states that gemm6_body's stores carry inside their
                        // inline asm, here around the builtin (the ring's loads are in flight, and hipcc counts vmcnt only for
                        // accesses it issued itself), fenced so that nothing is scheduled in between
                        __builtin_amdgcn_sched_barrier(0);
                        asm volatile("s_nop 4" ::: "memory");
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rc, c_l, (unsigned)((4 * mi * g.N + 16 * ct) * 16), 2);
                        asm volatile("s_nop 2" ::: "memory");
                        __builtin_amdgcn_sched_barrier(0);
                    }
            } else {
#pragma unroll
                for (int mi = 0; mi < 3; mi++)
#pragma unroll
                    for (int ct = 0; ct < 4; ct++)
#pragma unroll
                        for (int r = 0; r < 4; r++)
                            buf_store1_nt(acc[mi][ct][r] + bv[ct], rc, c_l, (unsigned)(((16 * mi + r) * g.N + 16 * ct) * 4));
            }
            SSTAMP(2)
        }
#ifdef PV_GEMM_STAMPS
        gs_acc[3]++;
#endif
    }
#ifdef PV_GEMM_STAMPS
    {   // [5], [6]: s_memtime and s_memrealtime (100 MHz) ticks of the whole item walk, for the clock the kernel ran at
        unsigned long long t1, r1;
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t1) :: "memory");
        asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(r1) :: "memory");
        gs_acc[5] = t1 - gs_t0;
        gs_acc[6] = r1 - gs_r0;
    }
    if (blockIdx.x == 0 && lane == 0)
        for (int i = 0; i < 8; i++) atomicAdd(&g_gemm_stamps[i], gs_acc[i]);
#endif
}

constexpr size_t LDS_GEMM = (size_t)2 * 4 * 256 * 32 * 2 + 2048 + 2048;   // 2 buffers x {A_hi, A_lo, W_hi, W_lo} x 256 rows x 32 bf16 = 128 KB, + two bias slots + completion flags
constexpr size_t LDS_GEMM6 = (size_t)2 * (2 * 256 + 3 * PV_GEMM6_BN) * 32 * 2 + 2048 + 2048;   // k_gemm_bf16x6: 2 buffers x ({A_hi, A_lo} x 256 rows + 3 W pieces x 128 rows) = 112 KB, + the same

}  // namespace

// iota[1024] per device (allocated once, never freed: 4 KB), the source of k_gemm_bf16x3's completion-flag transfers
static const unsigned* gemm_iota() {
    static std::mutex mu;
    static std::map<int, unsigned*> per_dev;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    auto it = per_dev.find(dev);
    if (it != per_dev.end()) return it->second;
    unsigned h[1024];
    for (unsigned i = 0; i < 1024; i++) h[i] = i;
    unsigned* d = nullptr;
    if (hipMalloc((void**)&d, sizeof h) != hipSuccess || hipMemcpy(d, h, sizeof h, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    per_dev[dev] = d;
    return d;
}

static void gemm_launch(pv_ctx* ctx, GemmArgs& g, hipStream_t st, int terms = 3) {
    g.tiles_m = (int)((g.M + PV_GEMM_TILE - 1) / PV_GEMM_TILE); g.tiles_n = g.N / (terms == 6 ? PV_GEMM6_BN : PV_GEMM_TILE);
    g.items = g.tiles_m * g.tiles_n * g.splits;
    const unsigned grid = (unsigned)(std::min((g.items + 7) / 8 * 8, (ctx->num_cu + 7) / 8 * 8));
    if (terms == 6) k_gemm_bf16x6<<<grid, 512, LDS_GEMM6, st>>>(g);
    else k_gemm_bf16x3<<<grid, 512, LDS_GEMM, st>>>(g);
}

// the shapes k_gemm_x6_stream takes (K is the kernel's constant; N: whole blocks of 64 columns per wave, the bias image in LDS)
static bool gemm_stream_shape(int N, int K, int splits) { return splits == 1 && K == GS_K && N % 512 == 0 && N <= GS_MAXN; }

static void gemm_stream_launch(pv_ctx* ctx, const float* A, const unsigned char* Ws, const float* bias, float* C, int64_t M, int N, int quads,
                               hipStream_t st) {
    GemmStreamArgs g;
    g.A = A; g.Ws = Ws; g.bias = bias; g.C = C; g.M = M; g.N = N; g.c_quads = quads;
    g.items = (int)((M + GS_ROWS - 1) / GS_ROWS);
    k_gemm_x6_stream<<<(unsigned)std::min(g.items, ctx->num_cu), 512, LDS_GEMM_STREAM, st>>>(g);
}

int pv_gemm_bf16x3_prepare() {
    PV_HIP(hipFuncSetAttribute((const void*)k_gemm_bf16x3, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_GEMM));
    PV_HIP(hipFuncSetAttribute((const void*)k_gemm_bf16x6, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_GEMM6));
    PV_HIP(hipFuncSetAttribute((const void*)k_gemm_x6_stream, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_GEMM_STREAM));
    PV_CHECK(gemm_iota() != nullptr, PV_ERR_HIP, "allocation of the GEMM's flag table failed");
    return PV_OK;
}

int pv_upload_split8(const float* w, size_t N, size_t K, unsigned char** d_split, std::vector<void*>& owned) {
    std::vector<uint16_t> sw;
    split8_rows(w, N, K, sw);
    return pv_dev_upload(sw, d_split, owned);
}

int pv_upload_split3(const float* w, size_t N, size_t K, unsigned char** d_planes, std::vector<void*>& owned) {
    std::vector<uint16_t> pl(3 * N * K);
    split3_planes(w, N, K, pl.data());
    return pv_dev_upload(pl, d_planes, owned);
}

int pv_upload_gemm6_stream(const float* w, size_t N, size_t K, unsigned char** d_stream, std::vector<void*>& owned) {
    std::vector<uint16_t> sw;
    pack_gemm6_stream(w, N, K, sw);
    return pv_dev_upload(sw, d_stream, owned);
}

int pv_gemm_bf16x3_async(pv_ctx* ctx, const pv_gemm_desc& d, hipStream_t st) {
    PV_CHECK(d.A && d.W && d.C && d.M > 0 && d.M % 4 == 0 && d.N % 256 == 0 && d.splits >= 1 && d.K % (32 * d.splits) == 0 &&
                 (!d.quads || d.splits == 1) && (d.terms == 0 || d.terms == 3 || d.terms == 6), PV_ERR_INVALID, "bad GEMM shape");
    pv_prof_scope ps(ctx, d.prof_name ? d.prof_name : (d.terms == 6 ? "k_gemm_bf16x6" : "k_gemm_bf16x3"), st);
    // the six-term product at K = 512 with the stream-ordered weights at hand: A resident in LDS, W streamed (k_gemm_x6_stream);
    // same C, bit for bit. Every other shape, and option p1_gemm6_stream = 0, keeps k_gemm_bf16x6.
    if (d.terms == 6 && d.W_stream && ctx->opt.p1_gemm6_stream && gemm_stream_shape(d.N, d.K, d.splits)) {
        gemm_stream_launch(ctx, reinterpret_cast<const float*>(d.A), d.W_stream, d.bias, d.C, d.M, d.N, d.quads, st);
        PV_HIP(hipGetLastError());
        return PV_OK;
    }
    GemmArgs g;
    g.A = d.A; g.W = d.W; g.bias = d.bias; g.C = d.C; g.M = d.M; g.N = d.N; g.K = d.K; g.splits = d.splits;
    g.c_quads = d.quads;
    g.iota = gemm_iota();
    PV_CHECK(g.iota, PV_ERR_HIP, "GEMM flag table missing");
    gemm_launch(ctx, g, st, d.terms == 6 ? 6 : 3);
    PV_HIP(hipGetLastError());
    return PV_OK;
}

// Diagnostic entry (tests, tuning): C = A . W^T + bias through k_gemm_bf16x3 alone. HOST pointers, fp32 row-major A [M,K],
// W [N,K], bias [N] or NULL, C [splits][M][N] row-major (quads = 0) or [M/4][N][4] (quads = 1, splits must be 1).
// M % 4 == 0, N % 256 == 0, K % (32 * splits) == 0. Returns the kernel time in ms through *ms when non-NULL.
constexpr int TERMS_STREAM = -6;   // debug_gemm: the six-term product through k_gemm_x6_stream
static int debug_gemm(pv_ctx* ctx, const float* A, const float* W, const float* bias, int64_t M, int N, int K, int splits, int quads,
                      float* C, float* ms, int terms) {
    PV_CHECK(ctx && A && W && C, PV_ERR_INVALID, "null argument");
    PV_CHECK(M > 0 && M % 4 == 0 && N % 256 == 0 && splits >= 1 && K % (32 * splits) == 0 && (!quads || splits == 1), PV_ERR_INVALID, "bad GEMM shape");
    PV_HIP(hipSetDevice(ctx->device));
    std::vector<void*> owned;
    unsigned char *dA = nullptr, *dW = nullptr;
    float *dB = nullptr, *dC = nullptr;
    int rc;
    auto cleanup = [&]() { for (void* p : owned) (void)hipFree(p); };
    if (terms == TERMS_STREAM) {   // A as plain fp32 rows, W as the fragment stream made at load time
        PV_CHECK(gemm_stream_shape(N, K, splits), PV_ERR_INVALID, "k_gemm_x6_stream: K = 512, N a multiple of 512 up to 2048, no split-K");
        float* fA = nullptr;
        if ((rc = pv_dev_upload(A, (size_t)M * K, &fA, owned)) || (rc = pv_upload_gemm6_stream(W, (size_t)N, (size_t)K, &dW, owned))) { cleanup(); return rc; }
        dA = reinterpret_cast<unsigned char*>(fA);
    } else if (terms == 6) {   // A as plain fp32 rows, W pre-split into three bf16 planes as at load time
        float* fA = nullptr;
        if ((rc = pv_dev_upload(A, (size_t)M * K, &fA, owned)) || (rc = pv_upload_split3(W, (size_t)N, (size_t)K, &dW, owned))) { cleanup(); return rc; }
        dA = reinterpret_cast<unsigned char*>(fA);
    } else if ((rc = pv_upload_split8(A, (size_t)M, (size_t)K, &dA, owned)) || (rc = pv_upload_split8(W, (size_t)N, (size_t)K, &dW, owned))) {
        cleanup();
        return rc;
    }
    if (bias && (rc = pv_dev_upload(bias, (size_t)N, &dB, owned))) { cleanup(); return rc; }
    // behind C a guard of one item's rows (256 x N floats, 0xff): a row stored past M - a replicated row of a ragged last
    // tile that its sized resource should have dropped - lands there and fails the call
    const size_t nc = (size_t)splits * M * N, ng = (size_t)PV_GEMM_TILE * N;
    if (hipMalloc((void**)&dC, (nc + ng) * sizeof(float)) != hipSuccess) { cleanup(); pv_set_error("hipMalloc failed"); return PV_ERR_HIP; }
    owned.push_back(dC);
    (void)hipMemset(dC, 0xff, (nc + ng) * sizeof(float));
    if (pv_gemm_bf16x3_prepare() != PV_OK) { cleanup(); return PV_ERR_HIP; }
    GemmArgs g;
    g.A = dA; g.W = dW; g.bias = dB; g.C = dC; g.M = M; g.N = N; g.K = K; g.splits = splits; g.c_quads = quads;
    g.iota = gemm_iota();
    if (!g.iota) { cleanup(); pv_set_error("GEMM flag table missing"); return PV_ERR_HIP; }
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    auto launch = [&]() {
        if (terms == TERMS_STREAM) gemm_stream_launch(ctx, reinterpret_cast<const float*>(dA), dW, dB, dC, M, N, quads, ctx->stream);
        else gemm_launch(ctx, g, ctx->stream, terms);
    };
    launch();   // warm
    (void)hipEventRecord(e0, ctx->stream);
    launch();
    (void)hipEventRecord(e1, ctx->stream);
    hipError_t er = hipStreamSynchronize(ctx->stream);
    float t = 0.f;
    (void)hipEventElapsedTime(&t, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (ms) *ms = t;
    if (er == hipSuccess) er = hipMemcpy(C, dC, nc * sizeof(float), hipMemcpyDeviceToHost);
    std::vector<uint32_t> guard(ng);
    if (er == hipSuccess) er = hipMemcpy(guard.data(), dC + nc, ng * sizeof(float), hipMemcpyDeviceToHost);
    cleanup();
    if (er != hipSuccess) { pv_set_error("GEMM failed: %s", hipGetErrorString(er)); return PV_ERR_HIP; }
    for (size_t i = 0; i < ng; i++)
        if (guard[i] != 0xffffffffu) { pv_set_error("GEMM stored past row M (guard word %zu behind C)", i); return PV_ERR_STATE; }
    return PV_OK;
}

extern "C" int pv_debug_gemm_bf16x3(pv_ctx* ctx, const float* A, const float* W, const float* bias, int64_t M, int N, int K,
                                    int splits, int quads, float* C, float* ms) {
    return debug_gemm(ctx, A, W, bias, M, N, K, splits, quads, C, ms, 3);
}
// the same through the 6-term form (k_gemm_bf16x6: fp32 A, split into three bf16 pieces in registers; W pre-split on the host
// into three bf16 planes by the function the model load uses)
extern "C" int pv_debug_gemm_bf16x6(pv_ctx* ctx, const float* A, const float* W, const float* bias, int64_t M, int N, int K,
                                    int splits, int quads, float* C, float* ms) {
    return debug_gemm(ctx, A, W, bias, M, N, K, splits, quads, C, ms, 6);
}

// the same product through k_gemm_x6_stream (W as the fragment stream of pack_gemm6_stream, made by the function the model load
// uses): K = 512, N a multiple of 512 up to 2048; C bit-identical to pv_debug_gemm_bf16x6's
extern "C" int pv_debug_gemm_x6_stream(pv_ctx* ctx, const float* A, const float* W, const float* bias, int64_t M, int N, int K,
                                       int quads, float* C, float* ms) {
    return debug_gemm(ctx, A, W, bias, M, N, K, 1, quads, C, ms, TERMS_STREAM);
}

#ifdef PV_GEMM_STAMPS
extern "C" int pv_debug_gemm_stamps(unsigned long long* out5) {
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    PV_HIP(hipDeviceSynchronize());
    PV_HIP(hipMemcpyFromSymbol(out5, HIP_SYMBOL(g_gemm_stamps), 8 * sizeof(unsigned long long)));
    PV_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_gemm_stamps), z, sizeof z));
    return PV_OK;
}
#endif
