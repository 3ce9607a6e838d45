// pv_opts.hpp — the options of a context. Plain C++ with no HIP dependency, so that host-only code (rnn_plan.hpp) can take it.
#pragma once

// Kernel-form choices of a context (pv_set_option / pv_get_option, include/pepper_hip.h). Defaults come from the
// environment ONCE, in pv_create (PV_LSTM_SPLIT, PV_LSTM_ROWS, PV_TAIL_ROWS, PV_HEAD_SPLITS, PV_HEAD_MAP, PV_GRU_ROWS,
// PV_GRU_SPLIT, PV_GRU_USPLIT, PV_SHARED_DEVICE, PV_P1_F32X6_MIN_BATCH); a forward call never reads the environment.
struct pv_opts {
    int lstm_split = 1;          // 0: never use the unit-split LSTM form
    int lstm_rows = 0;           // 0 auto, 16 or 32: tile form of k_lstm_layer (an explicit form also disables the unit split)
    int tail_rows = 0;           // 0 auto, 16 or 32
    int head_splits = 0;         // 0 auto, 1 / 3 / 11 / 33
    int head_map = 1;            // XCD-aware order of k_head_splitk
    int gru_rows = 0;            // 0 auto, 16 or 32
    int gru_split = 1;           // 0: neither split form of the GRU
    int gru_usplit = 1;          // 0: no unit-split form (the direction-split form stays)
    int shared_device = 0;       // 1: other work shares this GPU: no form that needs all its workgroups resident at once
    int exchange_spin_log2 = 18; // bounded polls of the split forms give up after 2^n tries (layer hand-offs: 2^(n+8))
    int debug_drop_part = -1;    // diagnostic: this part of a unit-split launch never runs (forces exchange time-outs)
    int p1_bf16_min_batch = 513; // PV_DTYPE_BF16_INPUT_GEMM, P1: calls with fewer windows run the fp32 kernels (faster there: 0.85 ms against
                                 // 1.0 for 512 windows; results then are the fp32 mode's); 0: always the bf16x3 kernels
    int p1_f32x6_min_batch = 2048; // PV_DTYPE_F32, P1: calls of at least this many windows (and no explicit lstm_rows) run the split-6
                                   // chain (fp32 products as six bf16 MFMA terms); smaller calls the fp32 kernels, bit for bit
                                   // (measured: 1.86 against 1.63 ms at 1024 windows, 2.07 against 2.64 at 1536)
    int p1_gemm6_stream = 1;     // split-6 chain: the decoder input projection as k_gemm_x6_stream (A tile resident in LDS, W streamed);
                                 // 0: as k_gemm_bf16x6 like every other six-term product. The results are the same bit for bit.
    int realign_scratch_kb = 512 << 10; // bounded pool of the realigner's direction bytes (pv_polish_realign*), in KB
};
