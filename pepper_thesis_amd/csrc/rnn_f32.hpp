// rnn_f32.hpp — the fp32 kernels of P1 (f32 MFMA) as the model's translation unit (rnn_p1.hip) sees them: a descriptor, an
// asynchronous launcher and a once-per-load `prepare` for the LSTM layers (rnn_lstm.hip) and for the head (rnn_head.hip), in the
// style of rnn_bf16.hpp. Which form a call takes is decided by its plan (rnn_plan.hpp); the launchers only fill arguments.
#pragma once
#include "pv_common.hpp"
#include "rnn_plan.hpp"

constexpr int PV_P1_T = 33;                          // time steps of a window
constexpr int PV_P1_F = 26;                          // image features per time step
constexpr int PV_P1_H = 256;                         // LSTM hidden units per direction
constexpr int PV_HEAD_K = PV_P1_T * 2 * PV_P1_H;     // inputs of linear_1: 16896

// ---- k_lstm_layer / k_lstm_split: one bidirectional LSTM layer (rnn_lstm.hip) -----------------------------------------------
struct pv_lstm_desc {
    int form;              // PV_LSTM_ROWS32 / PV_LSTM_ROWS16: k_lstm_layer on that tile; PV_LSTM_SPLIT4 / PV_LSTM_SPLIT2: k_lstm_split
    const int8_t* x_i8;    // encoder: images [B][33][26] (the layer is the encoder when this is set) ...
    const float* x_f32;    // ... decoder: the encoder's output [Bp][33][512]
    const float* wp;       // weights packed for `form` (pack_lstm of that tile / pack_lstm_split of that many parts)
    const float* bias;     // [2][1024] b_ih + b_hh
    float* out;            // [Bp][33][512]
    int64_t B;
    int n_tiles;           // 32-row tiles (Bp / 32)
    // k_lstm_split only: its exchange buffer (PV_LSTM_HX_BYTES, zeroed at load), the counters of the fence form
    // (PV_LSTM_FLAGS_BYTES, zeroed), the forward-call counter and the time-out word of the model
    void* hx;
    int* flags;
    const unsigned* epoch;
    int* err;
};
constexpr size_t PV_LSTM_HX_BYTES = (size_t)PV_SP_MAX_TILES * 2 * (2 * 2 * 1024) * 16;
constexpr size_t PV_LSTM_FLAGS_BYTES = (size_t)PV_SP_MAX_TILES * 2 * 4 * 32 * sizeof(int);
int pv_lstm_f32_async(pv_ctx* ctx, const pv_lstm_desc& d, hipStream_t st);
int pv_lstm_f32_prepare();

// ---- the head: linear_1 as a split-K product (k_head_splitk), then k_head_tail (rnn_head.hip) ----------------------------------
struct pv_head_splitk_desc {
    const float* dec;      // [Bp][33][512]
    const float* w1p;      // linear_1, pack_linear (32-row form)
    float* part;           // slabs [splits][B][512]
    int64_t B;
    int n_tiles;           // 32-row tiles
    int splits;            // divides 33
    int head_map;          // XCD-aware order of the workgroups
};
int pv_head_splitk_async(pv_ctx* ctx, const pv_head_splitk_desc& d, hipStream_t st);
// sum of slabs + bias + SELU, linear_2..5 + SELU, output layer, softmax; the last kernel of a forward call on every chain but
// the one that ends in k_tail_bf16
struct pv_head_tail_desc {
    int rows;              // 32 or 16 per workgroup
    const float* part;     // linear_1 slabs [splits][part_rows][512]
    int splits;
    int64_t part_rows;
    const float* b1;       // [512]
    const float* wp[4];    // linear_2..5, pack_linear in the form of `rows`
    const float* b[4];     // [512] each
    const float* wo;       // [3][512]
    const float* bo;       // [3]
    float* probs;          // [B][3]
    int64_t B;
    unsigned* epoch;       // bumped once (the forward-call counter of the unit-split LSTM form)
    const int* err;        // non-zero: the probabilities leave as NaN
};
int pv_head_tail_async(pv_ctx* ctx, const pv_head_tail_desc& d, hipStream_t st);
int pv_head_f32_prepare();
