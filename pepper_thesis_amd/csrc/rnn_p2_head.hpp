// rnn_p2_head.hpp — what every P2 (polisher) kernel form shares behind its dense1 product: the model's constants and the
// softmax / accumulate / argmax tail of the sliding loop (pepper/modules/python/models/predict.py:70-91). Device only, one
// copy: the fp32 persistent kernels (rnn_gru.hip) and the layer-wise bf16x3 path (rnn_rec_bf16.hip) use it.
#pragma once
#include <hip/hip_runtime.h>

namespace pvdev {

namespace p2 {
constexpr int SEQ = 1000, WIN = 100, JUMP = 50, NWIN = 19;   // columns of a chunk; windows of WIN columns, stride JUMP
constexpr int FEAT = 10, NCLS = 5;                           // pileup features per column, classes of dense1
constexpr int HG = 128;                                      // GRU hidden units per direction
}  // namespace p2

// ac[0..5) += softmax(lg); the raw logits go to row `lg_row` of logits [.][5] when that is not NULL (the last window of a call)
__device__ __forceinline__ void p2_softmax_acc(const float (&lg)[p2::NCLS], float* ac, float* logits, size_t lg_row) {
    float m = lg[0];
#pragma unroll
    for (int c = 1; c < p2::NCLS; c++) m = fmaxf(m, lg[c]);
    float e[p2::NCLS], sum = 0.0f;
#pragma unroll
    for (int c = 0; c < p2::NCLS; c++) { e[c] = expf(lg[c] - m); sum += e[c]; }
    const float inv = 1.0f / sum;
#pragma unroll
    for (int c = 0; c < p2::NCLS; c++) ac[c] += e[c] * inv;
    if (logits) {
#pragma unroll
        for (int c = 0; c < p2::NCLS; c++) logits[lg_row * p2::NCLS + c] = lg[c];
    }
}

// label of one column = argmax of its accumulated softmax, first maximum wins (torch.max, predict.py:91)
__device__ __forceinline__ int argmax5(const float* ac) {
    int best = 0;
    float bv = ac[0];
#pragma unroll
    for (int c = 1; c < p2::NCLS; c++) if (ac[c] > bv) { bv = ac[c]; best = c; }
    return best;
}

}  // namespace pvdev
