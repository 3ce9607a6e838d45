// rnn_plan.hpp — which kernel form an RNN call runs: every switch point of P1 and P2, and nothing else.
//
// Plain C++17 with no HIP dependency: pure functions of (dtype, batch, CU count, options). The launchers (rnn_p1.hip,
// rnn_gru.hip, rnn_rec_bf16.hip) plan first and then only allocate workspace, fill arguments and launch. tests/rnn_plan_shim.cpp
// compiles this header alone; tests/test_rnn_plan_cpu.py holds it against the Python restatement tests/rnn_forms.py.
#pragma once
#include <cstdint>

#include "../../include/pepper_hip.h"
#include "pv_opts.hpp"

// sizes the rules share with the kernels and launchers (each defined here only)
constexpr int PV_P1_ROWS = 32;                // the 32-row tile every P1 buffer and the head are counted in (one MFMA M-tile)
constexpr int64_t PV_P1_MAX_BATCH = 16384;    // windows per launch of the chains that materialise the decoder's input projections
constexpr int PV_SP_MAX_TILES = 64;           // 16-row tiles the unit-split exchange buffers are sized for (1024 windows)
constexpr int PV_HEAD_N = 512;                // outputs of linear_1
constexpr int PV_HEAD_MAX_SPLITS = 33;        // largest split-K factor of linear_1 (its K: 33 time steps = 528 steps of 32)
constexpr int PV_GEMM_TILE = 256;             // rows and columns of one work item of k_gemm_bf16x3 / k_gemm_bf16x6
constexpr int PV_TAIL_BF16_ROWS = 64;         // rows per workgroup of k_tail_bf16
constexpr int PV_P2_FOLD_MIN_BATCH = 2048;    // P2 bf16x3, 32-row forms: dense1 folds into the decoder from this many chunks on
// split-K factors of linear_1 as a GEMM (divisors of the 528 K steps), smallest first. The split-6 chain takes at least the 11
// slabs of k_head_splitk (shorter fp32 accumulation chains: with 4 slabs of 4224 the probabilities drift 1.8e-6 from the f32
// kernels)
constexpr int PV_LIN1_SPLITS_X6[] = {11, 12, 16, 22, 24, 33};
constexpr int PV_LIN1_SPLITS_BF16[] = {1, 2, 3, 4, 6, 8, 11, 12, 16, 22, 24, 33};

enum { PV_CHAIN_F32, PV_CHAIN_X6, PV_CHAIN_BF16X3 };   // k_lstm_* + k_head_splitk; the split-6 chain of the fp32 mode; bf16x3
enum { PV_LSTM_NONE, PV_LSTM_SPLIT4, PV_LSTM_SPLIT2, PV_LSTM_ROWS16, PV_LSTM_ROWS32 };   // k_lstm_split parts / k_lstm_layer tiles
enum { PV_TAIL_HEAD_TAIL, PV_TAIL_BF16 };

// one P1 launch (one chunk of a call)
struct pv_p1_plan {
    int chain, lstm;        // PV_CHAIN_*; PV_LSTM_* (f32 chain only, else PV_LSTM_NONE)
    int rows, mt;           // rows of a recurrent tile (16 / 32, 64 = mt 2); 32-row tiles per workgroup of k_rec_bf16 (0 on the f32 chain)
    int64_t Bp;             // padded rows: whole tiles
    int splits, head_map;   // split-K factor of linear_1; k_head_splitk in XCD-aware order
    int tail, tail_rows;    // PV_TAIL_*, its rows per workgroup
};

enum { PV_P2_US, PV_P2_DSPLIT, PV_P2_WG, PV_P2_GRU16, PV_P2_REC };   // fp32: k_gru_us, k_gru_p2 split / whole; bf16x3: k_gru16_bf16, k_rec_bf16

struct pv_p2_plan {
    int kind, rows, mt;   // PV_P2_*; tile rows (16 / 32 / 64); PV_P2_REC: 32-row tiles per workgroup, else 0
    int fold_dense;       // bf16x3: dense1 inside the decoder (k_p2_combine) instead of k_p2_dense's pass
    int64_t Bp;
};

// PV_DTYPE_F32 calls that take the split-6 chain: large enough (option p1_f32x6_min_batch) and no tile form forced
inline bool pv_p1_use_x6(int dtype, int64_t B, const pv_opts& o) {
    return dtype == PV_DTYPE_F32 && !o.lstm_rows && B >= o.p1_f32x6_min_batch;
}

// windows per launch of a P1 call of B windows. The bf16x3 mode and the split-6 chain materialise the decoder's input
// projections (33 x 8 KB per window: 4.4 GB at 16384 windows): larger calls run as chunks on the same stream
inline int64_t pv_p1_chunk(int dtype, int64_t B, const pv_opts& o) {
    return (dtype == PV_DTYPE_BF16_INPUT_GEMM || pv_p1_use_x6(dtype, B, o)) ? PV_P1_MAX_BATCH : B;
}

// linear_1 as a split-K GEMM into slabs [splits][Bp][512]: the first factor of the list whose work items fill the chip
template <int N> inline int pv_lin1_splits(const int (&factors)[N], int64_t Bp, int num_cu) {
    const int tiles = (int)((Bp + PV_GEMM_TILE - 1) / PV_GEMM_TILE) * (PV_HEAD_N / PV_GEMM_TILE);
    for (int f : factors)
        if (tiles * f >= num_cu) return f;
    return PV_HEAD_MAX_SPLITS;
}

inline pv_p1_plan pv_plan_p1(int dtype, int64_t B, int num_cu, const pv_opts& o) {
    pv_p1_plan p = {};
    const int n_tiles = (int)((B + PV_P1_ROWS - 1) / PV_P1_ROWS);
    p.head_map = o.head_map;
    // k_head_tail (PV_TAIL_HEAD_TAIL = 0): 16-row tiles unless 32-row tiles already fill the chip. On the X6 chain a 32-row
    // k_head_tail plan means the six-term form of the tail (k_tail_bf16<X6>, rnn_rec_bf16.hip: linear_2..5 on the bf16 MFMA,
    // the rest k_head_tail's arithmetic, the same profile scope); its 16-row plans run k_head_tail<16> itself
    p.tail_rows = o.tail_rows ? o.tail_rows : n_tiles >= num_cu ? 32 : 16;
    if (pv_p1_use_x6(dtype, B, o)) {   // 32-row tiles only: the 64-row form spills with three weight pieces
        p.chain = PV_CHAIN_X6; p.rows = 32; p.mt = 1; p.Bp = (int64_t)n_tiles * PV_P1_ROWS;
        p.splits = pv_lin1_splits(PV_LIN1_SPLITS_X6, p.Bp, num_cu);
        return p;
    }
    if (dtype == PV_DTYPE_BF16_INPUT_GEMM && B >= o.p1_bf16_min_batch) {   // (a small call is faster on the fp32 kernels below)
        // 64-row tiles (one weight fetch of the recurrent stream feeds twice the rows) once 32-row (tile, direction)
        // workgroups would not fit the chip at once
        p.chain = PV_CHAIN_BF16X3; p.mt = (int64_t)n_tiles * 2 > num_cu ? 2 : 1; p.rows = 32 * p.mt;
        p.Bp = (B + p.rows - 1) / p.rows * p.rows;
        p.splits = pv_lin1_splits(PV_LIN1_SPLITS_BF16, p.Bp, num_cu);
        // large batches: linear_2..5 as 3-term split products too (k_tail_bf16: 0.11 ms per 8192 windows against 0.27 for
        // k_head_tail); a small batch is a few workgroups each pulling the 4 MB of weights through one CU (0.30 ms for 64-512
        // windows), where k_head_tail's 16-row tiles spread the same fetch over four times the CUs (0.14 ms): it keeps those
        if ((B + PV_TAIL_BF16_ROWS - 1) / PV_TAIL_BF16_ROWS >= num_cu / 4) { p.tail = PV_TAIL_BF16; p.tail_rows = PV_TAIL_BF16_ROWS; }
        return p;
    }
    p.chain = PV_CHAIN_F32; p.Bp = (int64_t)n_tiles * PV_P1_ROWS;
    // unit-split form: one small fp32 batch whose (16-row tile, direction, part of the hidden units) workgroups all fit on
    // the chip at once: four parts up to 512 windows on 256 CUs, two parts up to 1024. Options lstm_split = 0, an explicit
    // lstm_rows, or shared_device = 1 (other work on this GPU: residency is not given) keep the one-workgroup form
    const int n_t16 = n_tiles * 2;
    const int parts = (int64_t)n_t16 * 2 * 4 <= num_cu ? 4 : 2;
    if (o.lstm_split && !o.lstm_rows && !o.shared_device && n_t16 <= PV_SP_MAX_TILES && (int64_t)n_t16 * 2 * parts <= num_cu) {
        p.lstm = parts == 4 ? PV_LSTM_SPLIT4 : PV_LSTM_SPLIT2; p.rows = 16;
    } else {
        // 32-row tiles once (tile, direction) workgroups fill the chip, else 16-row tiles: twice the workgroups, half the
        // MFMA cycles per time step
        p.rows = o.lstm_rows ? o.lstm_rows : (int64_t)n_tiles * 2 >= num_cu ? 32 : 16;
        p.lstm = p.rows == 32 ? PV_LSTM_ROWS32 : PV_LSTM_ROWS16;
    }
    // k_head_splitk: 11 slabs of 3 time steps; 33 single-step slabs only for batches too small to fill the chip
    p.splits = o.head_splits ? o.head_splits : (int64_t)n_tiles * 11 >= num_cu ? 11 : PV_HEAD_MAX_SPLITS;
    return p;
}

inline pv_p2_plan pv_plan_p2(int dtype, int64_t B, int num_cu, const pv_opts& o) {
    pv_p2_plan p = {};
    if (dtype == PV_DTYPE_BF16_INPUT_GEMM) {
        // 16-row tiles (k_gru16_bf16: half the MFMA and cell-update time per step) while every (tile, direction) workgroup has
        // a CU of its own (up to 2048 chunks on 256 CUs: 13.2 ms against 17.9 at 2048). Beyond that, two 16-row tiles per
        // workgroup measured no better than the 32-row form - 6.0 / 6.3 ms against 6.0 / 6.8 per 19 windows at 2121 chunks -
        // and cannot fold dense1 in: not used. 64-row tiles (mt 2: one weight fetch feeds twice the rows) once 32-row
        // workgroups would need more than two rounds of the chip; below that 32-row tiles keep more CUs busy
        p.kind = ((B + 15) / 16) * 2 <= (int64_t)num_cu ? PV_P2_GRU16 : PV_P2_REC;
        p.mt = p.kind == PV_P2_GRU16 ? 0 : ((B + 31) / 32) * 2 > 2 * (int64_t)num_cu ? 2 : 1;
        p.rows = p.kind == PV_P2_GRU16 ? 16 : 32 * p.mt;
        // dense1 as one more MFMA tile of the decoder's steps (partial logits, 105 MB per window at 4096 chunks, summed by
        // k_p2_combine) instead of the decoder's split8 output (420 MB) and k_p2_dense's pass over it: 24.9 -> 23.9 ms at 4096
        // chunks. It lengthens every decoder step by ~5 %, which is all a small batch of the 32-row forms sees (64 chunks:
        // 12.3 -> 12.6 ms), so those keep the separate pass; the 16-row form gains at every size (64 chunks 6.22 -> 6.14 ms,
        // 2048 chunks 12.1 -> 11.0)
        p.fold_dense = p.kind == PV_P2_GRU16 || B >= PV_P2_FOLD_MIN_BATCH;
    } else {
        // 32-row tiles once they fill the chip, else 16-row tiles (twice the workgroups, half the time per step)
        p.rows = o.gru_rows ? o.gru_rows : (B + 31) / 32 >= num_cu ? 32 : 16;
        const int64_t n_tiles = (B + p.rows - 1) / p.rows;
        // the split forms need every workgroup resident at once: options gru_split = 0 or shared_device = 1 keep one workgroup
        // per tile. Unit split (tile, direction, half of the units; gru_usplit = 0 turns it off) up to 1024 chunks on 256 CUs;
        // direction split (the launch is a chain of dependent steps, and a step then carries one direction's MFMAs per SIMD
        // instead of two) while every (tile, direction) workgroup has a CU of its own
        const bool may_split = p.rows == 16 && o.gru_split && !o.shared_device;
        p.kind = may_split && o.gru_usplit && 4 * n_tiles <= num_cu ? PV_P2_US : may_split && 2 * n_tiles <= num_cu ? PV_P2_DSPLIT : PV_P2_WG;
    }
    p.Bp = (B + p.rows - 1) / p.rows * p.rows;
    return p;
}
