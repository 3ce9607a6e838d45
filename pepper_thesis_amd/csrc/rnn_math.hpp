// rnn_math.hpp — the activation helpers of the recurrent kernels (rnn_lstm.hip, rnn_head.hip, rnn_gru.hip, rnn_rec_bf16.hip),
// device only, one copy.
#pragma once
#include <hip/hip_runtime.h>

namespace pvdev {

// v_exp_f32 / v_rcp_f32 (1 ulp) instead of the IEEE division sequence: ~3x fewer VALU instructions in the
// cell update; absolute error of sigmoid/tanh stays ~1e-7 (tests pin 2e-5 on layer outputs).
__device__ __forceinline__ float rcpf_(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float sigmoidf_(float x) { return rcpf_(1.0f + __expf(-x)); }
// tanh = 1 - 2/(e^{2x}+1): saturates cleanly at +-1 (e = inf -> 1, e = 0 -> -1). TWO spellings, and every kernel keeps the one
// it was written with:
//   tanhf_fma_   the fused multiply-add spelled out: k_lstm_layer, k_lstm_split (rnn_lstm.hip)
//   tanhf_       left to the compiler's contraction: k_gru_* (rnn_gru.hip), k_rec_bf16 / k_gru16_bf16 (rnn_rec_bf16.hip)
// They are not merged: the compiler schedules the two differently (rewriting rnn_gru.hip and rnn_rec_bf16.hip to the fmaf
// form changes 1759 and 239 lines of their instruction text), and the outputs of these kernels are compared bit for bit
// between kernel forms (tests/test_rnn_forms_gpu.py). One form for all is a change of generated code, to be made and
// measured on its own.
__device__ __forceinline__ float tanhf_fma_(float x) {
    const float e = __expf(2.0f * x);
    return __builtin_fmaf(-2.0f, rcpf_(e + 1.0f), 1.0f);
}
__device__ __forceinline__ float tanhf_(float x) {
    const float e = __expf(2.0f * x);
    return 1.0f - 2.0f * rcpf_(e + 1.0f);
}
// c' = f * c + i * g with the fused multiply-add spelled out: left to the compiler's contraction, two instantiations of the
// same cell update (k_lstm_layer / k_lstm_split) can round differently, and their outputs are compared bit for bit
__device__ __forceinline__ float lstm_c_(float fg, float c, float ig, float gg) { return __builtin_fmaf(fg, c, ig * gg); }
__device__ __forceinline__ float seluf_(float x) {
    return 1.0507009873554805f * (x > 0.0f ? x : 1.6732632423543772f * (__expf(x) - 1.0f));
}

}  // namespace pvdev
