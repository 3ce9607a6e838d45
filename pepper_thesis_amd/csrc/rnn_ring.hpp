// rnn_ring.hpp — the weight-fragment rings of the fp32 P1 kernels on the f32 MFMA: k_lstm_layer (rnn_lstm.hip), k_head_splitk
// and k_head_tail (rnn_head.hip). Device only. Fragment layouts: mfma_tiles.hpp; the streams they read: pack_lstm,
// pack_linear (rnn_pack_host.hpp).
#pragma once
#include "mfma_tiles.hpp"

namespace pvdev {

// ---- weight-fragment rings ------------------------------------------------------------------------------------------
// The B operand (packed weights, one f32x4 per lane per gate tile per k-block of 8) comes from L2, ~1 us away, while a
// k-block is 12-16 MFMAs (0.3-0.45 us): fragments run in a ring of FOUR register sets fed by raw buffer loads THREE
// k-blocks ahead. `sched_barrier` fences keep hipcc from sinking the prefetches back next to their uses. A fragments come
// from LDS one block ahead.

// Recurrent form, acc[nt] += [A1 | A2] . B: k-blocks [0,nkb1) read A1 (x_t), [nkb1,nkb1+nkb2) read A2 (h_{t-1}); the packed
// weight stream is contiguous over both. The ring wraps into the next time step (same weights every step), so `bq` slots
// 0..2 must hold k-blocks 0..2 on entry and do so again on exit: a step never starts with a cold L2 round trip.
// (nkb1 + nkb2) % 4 == 0.
template <int TR, int NT>
__device__ __forceinline__ void mma_dual_ringb(Gate<TR> (&acc)[NT], const float* __restrict__ A1, int lda1, int nkb1,
                                               const float* __restrict__ A2, int lda2, int nkb2,
                                               __amdgpu_buffer_rsrc_t wr, f32x4 (&bq)[4][NT], int lane) {
    typedef typename AFrag<TR>::type afrag;
    constexpr int NJ = TR == 32 ? 4 : 2;
    const float* ap1 = afrag_ptr<TR>(A1, lda1, lane);
    const float* ap2 = afrag_ptr<TR>(A2, lda2, lane) - 8 * nkb1;
    const int nkb = nkb1 + nkb2;
    const unsigned lane16 = (unsigned)lane * 16u;
    afrag aq[2];
#define RB_B(slot, kbv) { _Pragma("unroll") for (int nt = 0; nt < NT; nt++) bq[slot][nt] = buf_load4(wr, lane16, (unsigned)(((kbv) * NT + nt) * 1024)); }
#define RB_A(slot, kbv) { aq[slot] = *reinterpret_cast<const afrag*>(((kbv) < nkb1 ? ap1 : ap2) + 8 * (kbv)); }
#define RB_M(bs, as)                                                                    \
    {                                                                                   \
        _Pragma("unroll") for (int j = 0; j < NJ; j++)                                  \
            _Pragma("unroll") for (int nt = 0; nt < NT; nt++) gate_mma<TR>(acc[nt], aq[as], bq[bs][nt], j); \
    }
#define RB_F __builtin_amdgcn_sched_barrier(0);
    RB_A(0, 0)
#pragma nounroll
    for (int kb = 0; kb < nkb; kb += 4) {
        const int kw = kb + 4 < nkb ? kb + 4 : 0;
        RB_B(3, kb + 3) RB_A(1, kb + 1) RB_F RB_M(0, 0) RB_F
        RB_B(0, kw) RB_A(0, kb + 2) RB_F RB_M(1, 1) RB_F
        RB_B(1, kw + 1) RB_A(1, kb + 3) RB_F RB_M(2, 0) RB_F
        RB_B(2, kw + 2)
        if (kb + 4 < nkb) RB_A(0, kb + 4)
        RB_F RB_M(3, 1) RB_F
    }
#undef RB_B
#undef RB_A
#undef RB_M
#undef RB_F
}

// Single-operand form over a CONTINUING weight stream: multiplies k-blocks [kpos, kpos + nkb) of the stream behind `wr`
// with A[TR x 8*nkb] in LDS. On entry bq slots 0..2 hold k-blocks kpos..kpos+2; on exit they hold kpos+nkb..kpos+nkb+2,
// i.e. the next call's first blocks, so consecutive calls (time steps of linear_1) never start with a cold L2/HBM round
// trip. Requests beyond the resource's size return zeros. nkb % 4 == 0. Fragment layouts: mfma_tiles.hpp (the K order
// inside a k-block is a permutation of 0..7, which only changes the fp32 summation order).
template <int TR, int NT>
__device__ __forceinline__ void mma_stream_ringb(Gate<TR> (&acc)[NT], const float* __restrict__ A, int lda, int nkb,
                                                 __amdgpu_buffer_rsrc_t wr, int kpos, f32x4 (&bq)[4][NT], int lane) {
    typedef typename AFrag<TR>::type afrag;
    constexpr int NJ = TR == 32 ? 4 : 2;
    const float* ap = afrag_ptr<TR>(A, lda, lane);
    const unsigned lane16 = (unsigned)lane * 16u;
    afrag aq[2];
#define RB_B(slot, kbv) { _Pragma("unroll") for (int nt = 0; nt < NT; nt++) bq[slot][nt] = buf_load4(wr, lane16, (unsigned)(((kpos + (kbv)) * NT + nt) * 1024)); }
#define RB_A(slot, kbv) { aq[slot] = *reinterpret_cast<const afrag*>(ap + 8 * (kbv)); }
#define RB_M(bs, as)                                                                    \
    {                                                                                   \
        _Pragma("unroll") for (int j = 0; j < NJ; j++)                                  \
            _Pragma("unroll") for (int nt = 0; nt < NT; nt++) gate_mma<TR>(acc[nt], aq[as], bq[bs][nt], j); \
    }
#define RB_F __builtin_amdgcn_sched_barrier(0);
    RB_A(0, 0)
#pragma nounroll
    for (int kb = 0; kb < nkb; kb += 4) {
        RB_B(3, kb + 3) RB_A(1, kb + 1) RB_F RB_M(0, 0) RB_F
        RB_B(0, kb + 4) RB_A(0, kb + 2) RB_F RB_M(1, 1) RB_F
        RB_B(1, kb + 5) RB_A(1, kb + 3) RB_F RB_M(2, 0) RB_F
        RB_B(2, kb + 6)
        if (kb + 4 < nkb) RB_A(0, kb + 4)
        RB_F RB_M(3, 1) RB_F
    }
#undef RB_B
#undef RB_A
#undef RB_M
#undef RB_F
}
template <int NT>
__device__ __forceinline__ void ring_prime(f32x4 (&bq)[4][NT], __amdgpu_buffer_rsrc_t wr, int kpos, int lane) {
#pragma unroll
    for (int q = 0; q < 3; q++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++) bq[q][nt] = buf_load4(wr, (unsigned)lane * 16u, (unsigned)(((kpos + q) * NT + nt) * 1024));
}

}  // namespace pvdev
