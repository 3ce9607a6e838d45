// rnn_pack_host.hpp — host-only: PyTorch-layout weights -> the operand layouts the recurrent kernels read, made once at load time.
// Every function here is a pure function from weights to a vector. No HIP, and no header of the library beyond the piece
// rule (split3_host.hpp) and the pv_rnn_dir declaration: the tests compile it alone (tests/rnn_pack_shim.cpp) and hold every
// layout against a numpy restatement of its comment (tests/test_rnn_pack_host_cpu.py). The launchers upload what comes out
// (pv_dev_upload, pv_common.hpp).
//
//   fp32 fragments, f32 MFMA    pack_lstm, pack_lstm_split, pack_linear (P1: rnn_lstm.hip, rnn_head.hip)
//                               pack_gru, pack_gru_us (P2: rnn_gru.hip)
//   bf16 pieces, bf16 MFMA      pack_rec_bf16, pack_rec_x6_16, pack_gru16_bf16, pack_tail_bf16, pack_tail_x6, pack_p2_dense, pack_p2_dense16 (rnn_rec_bf16.hip)
//   GEMM operands               split8_rows (k_gemm_bf16x3); the three planes of k_gemm_bf16x6 are split3_planes (split3_host.hpp);
//                               pack_gemm6_stream (k_gemm_x6_stream)
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/pepper_hip.h"
#include "split3_host.hpp"

constexpr int PV_PACK_LSTM_H = 256;   // hidden units of P1's LSTM layers
constexpr int PV_PACK_GRU_H = 128;    // hidden units of P2's GRU layers
constexpr int PV_PACK_NCLS = 5;       // classes of P2's dense layer
constexpr int PV_PACK_HEAD_N = 512;   // width of P1's linear_2..5

// element (n, k) of one direction's [W_ih (K real columns, padded to KP) | W_hh (HID columns)]
static inline float pack_wval(const pv_rnn_dir& dir, int K, int KP, int HID, int n, int k) {
    if (k < KP) return k < K ? dir.w_ih[(size_t)n * K + k] : 0.0f;
    return dir.w_hh[(size_t)n * HID + (k - KP)];
}

// A slot of bf16 fragments is 1 KB per piece: piece q of value (lane, j) sits at 2-byte index 512 q + 8 lane + j. The pieces are
// the first `pieces` of split3_bits: (hi, lo) = (x0, x1) of the two-piece operands, all three for the split-6 form.
static inline void pack_put_pieces(uint16_t* slot, int lane, int j, float v, int pieces = 2) {
    uint16_t p[3];
    split3_bits(v, p);
    for (int q = 0; q < pieces; q++) slot[512 * q + lane * 8 + j] = p[q];
}

// Operand format of the bf16x3 GEMMs ("split8"): every 8 consecutive K elements of a row are stored as 32 bytes,
// 8 x bf16 hi followed by 8 x bf16 lo, with x ~= hi + lo, hi = bf16(x), lo = bf16(x - hi) (round to nearest even twice).
// One 16-byte half of a group is exactly one MFMA A/B fragment of v_mfma_f32_32x32x16_bf16, so the GEMM moves operands
// from HBM to LDS by LDS-DMA without touching a register. Byte offset of element k inside a row: (k >> 3) * 32 + (k & 7) * 2
// (+16 for lo).
// w [N, K] row-major -> split8 rows of K * 4 bytes, K % 8 == 0
static inline void split8_rows(const float* w, size_t N, size_t K, std::vector<uint16_t>& out) {
    out.assign(2 * N * K, 0);
    for (size_t r = 0; r < N; r++)
        for (size_t k = 0; k < K; k++) {
            uint16_t p[3];
            split3_bits(w[r * K + k], p);
            const size_t o = r * K * 2 + (k >> 3) * 16 + (k & 7);   // in 2-byte units
            out[o] = p[0];
            out[o + 8] = p[1];
        }
}

// ---- fp32 fragments of the f32 MFMA ----------------------------------------------------------------------------------
// LSTM layer (k_lstm_layer), 8 waves per workgroup, wave w owns hidden units [32w, 32w+32) of the gates i,f,g,o (nt).
// wp [2 dirs][8 waves][k-block of 8][gate][lane][4]; K = [x (padded to KP) | h]; bias [2][1024] = b_ih + b_hh. Tile forms as in
// mfma_tiles.hpp:
//  32 rows: lane -> gate column nt*H + 32w + (lane&31); values k = 8kb + 4*(lane>>5) + j, j = 0..3
//  16 rows: lane -> columns nt*H + 32w + 16t + (lane&15), t = 0,1; values {t0 j0, t0 j1, t1 j0, t1 j1}, k = 8kb + 2*(lane>>4) + j
static inline void pack_lstm(const pv_rnn_dir* dirs, int K, int KP, int TR, std::vector<float>& wp, std::vector<float>& bias) {
    constexpr int H = PV_PACK_LSTM_H;
    const int nkb = (KP + H) / 8, NT = 4, NW = 8;
    wp.assign((size_t)2 * NW * nkb * NT * 256, 0.0f);
    bias.assign((size_t)2 * 4 * H, 0.0f);
    for (int d = 0; d < 2; d++) {
        for (int n = 0; n < 4 * H; n++) bias[(size_t)d * 4 * H + n] = dirs[d].b_ih[n] + dirs[d].b_hh[n];
        auto wval = [&](int n, int k) { return pack_wval(dirs[d], K, KP, H, n, k); };
        for (int w = 0; w < NW; w++)
            for (int kb = 0; kb < nkb; kb++)
                for (int nt = 0; nt < NT; nt++)
                    for (int lane = 0; lane < 64; lane++) {
                        float* dst = &wp[((((size_t)(d * NW + w) * nkb + kb) * NT + nt) * 64 + lane) * 4];
                        if (TR == 32) {
                            for (int j = 0; j < 4; j++) dst[j] = wval(nt * H + 32 * w + (lane & 31), kb * 8 + 4 * (lane >> 5) + j);
                        } else {
                            for (int t = 0; t < 2; t++)
                                for (int j = 0; j < 2; j++)
                                    dst[2 * t + j] = wval(nt * H + 32 * w + 16 * t + (lane & 15), kb * 8 + 2 * (lane >> 4) + j);
                        }
                    }
    }
}

// unit-split form (k_lstm_split), SP_NS parts of 16 / SP_NS waves: [dir][part][wave][k-block of 8][2][lane][4] =
// {i j0, i j1, f j0, f j1}, {g j0, g j1, o j0, o j1} with W[gate*H + (H/SP_NS)*part + 16*wave + (lane&15)][8kb + 2*(lane>>4) + j],
// K = [x (padded) | h]
static inline void pack_lstm_split(const pv_rnn_dir* dirs, int K, int KP, int SP_NS, std::vector<float>& wp) {
    constexpr int H = PV_PACK_LSTM_H;
    const int nkb = (KP + H) / 8, NW = 16 / SP_NS, UPP = H / SP_NS;
    wp.assign((size_t)2 * 16 * nkb * 2 * 256, 0.0f);
    for (int d = 0; d < 2; d++) {
        auto wval = [&](int n, int k) { return pack_wval(dirs[d], K, KP, H, n, k); };
        for (int p = 0; p < SP_NS; p++)
            for (int w = 0; w < NW; w++)
                for (int kb = 0; kb < nkb; kb++)
                    for (int half = 0; half < 2; half++)
                        for (int lane = 0; lane < 64; lane++) {
                            float* dst = &wp[(((((size_t)(d * SP_NS + p) * NW + w) * nkb + kb) * 2 + half) * 64 + lane) * 4];
                            const int u = UPP * p + 16 * w + (lane & 15);
                            for (int gg = 0; gg < 2; gg++)
                                for (int j = 0; j < 2; j++)
                                    dst[2 * gg + j] = wval((2 * half + gg) * H + u, kb * 8 + 2 * (lane >> 4) + j);
                        }
    }
}

// Linear [512, K] (k_head_splitk, k_head_tail): [4 waves][k-block of 8][4][lane][4]; wave w owns columns [128w, 128w+128) as four
// 32-column "gate tiles" nt; tile forms as in pack_lstm
static inline void pack_linear(const float* W, int K, int TR, std::vector<float>& wp) {
    const int nkb = K / 8;
    wp.assign((size_t)4 * nkb * 4 * 256, 0.0f);
    for (int w = 0; w < 4; w++)
        for (int kb = 0; kb < nkb; kb++)
            for (int nt = 0; nt < 4; nt++)
                for (int lane = 0; lane < 64; lane++) {
                    float* dst = &wp[((((size_t)w * nkb + kb) * 4 + nt) * 64 + lane) * 4];
                    if (TR == 32) {
                        const int n = 128 * w + 32 * nt + (lane & 31);
                        for (int j = 0; j < 4; j++) dst[j] = W[(size_t)n * K + kb * 8 + 4 * (lane >> 5) + j];
                    } else {
                        for (int t = 0; t < 2; t++)
                            for (int j = 0; j < 2; j++)
                                dst[2 * t + j] = W[(size_t)(128 * w + 32 * nt + 16 * t + (lane & 15)) * K + kb * 8 + 2 * (lane >> 4) + j];
                    }
                }
}

// GRU layer (k_gru_p2), 4 waves per direction, wave w owns hidden units [32w, 32w+32) of the gates r,z,n (nt).
// wp [2 dirs][4 waves][k-block of 8][gate r,z,n][lane][4]; K = [x (padded to KP) | h]; bias [2][4][128] = b_ir + b_hr, b_iz + b_hz,
// b_in, b_hn.
//  32-row form: lane -> gate column 32w + (lane&31), the four values are k = 8kb + 4*(lane>>5) + j, j = 0..3
//  16-row form: lane -> gate columns 32w + (lane&15) (tile 0) and 32w + 16 + (lane&15) (tile 1),
//               the four values are {tile0 j0, tile0 j1, tile1 j0, tile1 j1} with k = 8kb + 2*(lane>>4) + j
// hx_order: the stream starts with the h-part k-blocks ([h | x], the order of the overlapped window form) instead of [x | h]
static inline void pack_gru(const pv_rnn_dir* dirs, int K, int KP, int TR, std::vector<float>& wp, std::vector<float>& bias, bool hx_order = false) {
    constexpr int HG = PV_PACK_GRU_H;
    const int nkb = (KP + HG) / 8;
    wp.assign((size_t)2 * 4 * nkb * 3 * 256, 0.0f);
    bias.assign((size_t)2 * 4 * HG, 0.0f);
    for (int d = 0; d < 2; d++) {
        for (int u = 0; u < HG; u++) {
            bias[(size_t)d * 4 * HG + 0 * HG + u] = dirs[d].b_ih[0 * HG + u] + dirs[d].b_hh[0 * HG + u];
            bias[(size_t)d * 4 * HG + 1 * HG + u] = dirs[d].b_ih[1 * HG + u] + dirs[d].b_hh[1 * HG + u];
            bias[(size_t)d * 4 * HG + 2 * HG + u] = dirs[d].b_ih[2 * HG + u];
            bias[(size_t)d * 4 * HG + 3 * HG + u] = dirs[d].b_hh[2 * HG + u];
        }
        auto wval = [&](int n, int k) {
            if (hx_order) k = k < HG ? KP + k : k - HG;   // stream position -> position in [x | h]
            return pack_wval(dirs[d], K, KP, HG, n, k);
        };
        for (int w = 0; w < 4; w++)
            for (int kb = 0; kb < nkb; kb++)
                for (int nt = 0; nt < 3; nt++)
                    for (int lane = 0; lane < 64; lane++) {
                        float* dst = &wp[((((size_t)(d * 4 + w) * nkb + kb) * 3 + nt) * 64 + lane) * 4];
                        if (TR == 32) {
                            const int n = nt * HG + 32 * w + (lane & 31);
                            for (int j = 0; j < 4; j++) dst[j] = wval(n, kb * 8 + 4 * (lane >> 5) + j);
                        } else {
                            for (int t = 0; t < 2; t++)
                                for (int j = 0; j < 2; j++)
                                    dst[2 * t + j] = wval(nt * HG + 32 * w + 16 * t + (lane & 15), kb * 8 + 2 * (lane >> 4) + j);
                        }
                    }
    }
}

// unit-split form (k_gru_us): [dir][half][wave][pair of k-blocks][gate r,z,n][lane][4], stream order [h | x]; lane -> unit
// 64 half + 16 wave + (lane&15), the four values are k = 16 pair + 8 kh + 2*(lane>>4) + j, (kh, j) = (0,0), (0,1), (1,0), (1,1)
static inline void pack_gru_us(const pv_rnn_dir* dirs, int K, int KP, std::vector<float>& wp) {
    constexpr int HG = PV_PACK_GRU_H;
    const int np = (KP + HG) / 16;
    wp.assign((size_t)2 * 2 * 4 * np * 3 * 256, 0.0f);
    for (int d = 0; d < 2; d++) {
        auto wval = [&](int n, int kpos) -> float {   // kpos: position in the [h | x] stream
            if (kpos < HG) return dirs[d].w_hh[(size_t)n * HG + kpos];
            const int k = kpos - HG;
            return k < K ? dirs[d].w_ih[(size_t)n * K + k] : 0.0f;
        };
        for (int hf = 0; hf < 2; hf++)
            for (int w = 0; w < 4; w++)
                for (int pp = 0; pp < np; pp++)
                    for (int g = 0; g < 3; g++)
                        for (int lane = 0; lane < 64; lane++) {
                            float* dst = &wp[(((((size_t)(d * 2 + hf) * 4 + w) * np + pp) * 3 + g) * 64 + lane) * 4];
                            const int n = g * HG + 64 * hf + 16 * w + (lane & 15);
                            for (int kh = 0; kh < 2; kh++)
                                for (int j = 0; j < 2; j++) dst[2 * kh + j] = wval(n, 16 * pp + 8 * kh + 2 * (lane >> 4) + j);
                        }
    }
}

// ---- bf16 pieces of the bf16 MFMA (slots: pack_put_pieces) ---------------------------------------------------------------
// k_rec_bf16. Fragment stream of one (direction, wave): slots [x-part k-steps x gates | h-part k-steps x gates]; a slot is 1 KB of
// hi fragments followed by 1 KB of lo fragments (pieces = 3, LSTM only: x0 | x1 | x2, the split-6 form of the -DPV_REC_X6_MFMA32 build); lane -> weight row
// gate * HID + 32 * wave + (lane & 31), 8 consecutive K values 16 * ks + 8 * (lane >> 5) + j (the B operand of
// v_mfma_f32_32x32x16_bf16). cell = 4: LSTM, hidden 256, two x-part k-steps; cell = 3: GRU, hidden 128, and with kx > 0 (the
// encoder) the x-part, one k-step, goes to a stream of its own, wx [dir][wave][gate] slots of 2 KB. kx = real input features
// (features beyond them are zero) or 0: no x-part.
static inline void pack_rec_bf16(const pv_rnn_dir* dirs, int cell, int kx, int pieces, std::vector<uint16_t>& wp, std::vector<uint16_t>& wx) {
    const int NG = cell, HID = cell == 4 ? PV_PACK_LSTM_H : PV_PACK_GRU_H, NW = HID / 32, KS_H = HID / 16;
    const int KS_X = kx ? (cell == 4 ? 2 : 1) : 0;
    const bool xres = kx && cell == 3;
    const int nslot = (xres ? 0 : KS_X * NG) + KS_H * NG;
    const size_t SL = (size_t)pieces * 512;   // 2-byte units of one slot: a 1 KB fragment per piece
    wp.assign((size_t)2 * NW * nslot * SL, 0);
    wx.assign(xres ? (size_t)2 * NW * NG * 1024 : 0, 0);
    for (int d = 0; d < 2; d++)
        for (int w = 0; w < NW; w++) {
            auto fill = [&](uint16_t* dst, bool xpart, int ks, int g) {
                for (int lane = 0; lane < 64; lane++)
                    for (int j = 0; j < 8; j++) {
                        const int n = g * HID + 32 * w + (lane & 31), k = 16 * ks + 8 * (lane >> 5) + j;
                        float v;
                        if (xpart) v = k < kx ? dirs[d].w_ih[(size_t)n * kx + k] : 0.0f;
                        else v = dirs[d].w_hh[(size_t)n * HID + k];
                        pack_put_pieces(dst, lane, j, v, pieces);
                    }
            };
            uint16_t* base = wp.data() + (size_t)(d * NW + w) * nslot * SL;
            int slot = 0;
            if (!xres)
                for (int ks = 0; ks < KS_X; ks++)
                    for (int g = 0; g < NG; g++) fill(base + (size_t)(slot++) * SL, true, ks, g);
            for (int ks = 0; ks < KS_H; ks++)
                for (int g = 0; g < NG; g++) fill(base + (size_t)(slot++) * SL, false, ks, g);
            if (xres)
                for (int g = 0; g < NG; g++) fill(wx.data() + ((size_t)(d * NW + w) * NG + g) * 1024, true, 0, g);
        }
}

// Split-6 LSTM form of k_rec_bf16 on v_mfma_f32_16x16x32_bf16 (ring_x6_16). Fragment stream of one (direction, wave): slots
// [x-part: gate, half | h-part: k-step of 32, gate, half], every slot three 1 KB pieces x0 | x1 | x2; lane -> weight row
// gate * 256 + 32 * wave + 16 * half + (lane & 15), 8 consecutive K values 32 * ks + 8 * (lane >> 4) + j. kx > 0 (the encoder):
// the x-part is ONE k-step (features beyond kx zero), 8 slots in front of the 64 of W_hh; kx = 0: no x-part. (A 16-column x 32-k
// fragment is as many weights as a 32-column x 16-k one of pack_rec_bf16: the stream is the same 72 / 64 slots long.)
static inline void pack_rec_x6_16(const pv_rnn_dir* dirs, int kx, std::vector<uint16_t>& wp) {
    constexpr int HID = PV_PACK_LSTM_H, NW = HID / 32, KS_H = HID / 32, NG = 4;
    const int nslot = (kx ? NG * 2 : 0) + KS_H * NG * 2;
    constexpr size_t SL = 3 * 512;
    wp.assign((size_t)2 * NW * nslot * SL, 0);
    for (int d = 0; d < 2; d++)
        for (int w = 0; w < NW; w++) {
            uint16_t* dst = wp.data() + (size_t)(d * NW + w) * nslot * SL;
            for (int ks = kx ? -1 : 0; ks < KS_H; ks++)   // -1: the x-part
                for (int g = 0; g < NG; g++)
                    for (int c = 0; c < 2; c++, dst += SL)
                        for (int lane = 0; lane < 64; lane++)
                            for (int j = 0; j < 8; j++) {
                                const int n = g * HID + 32 * w + 16 * c + (lane & 15), k = 8 * (lane >> 4) + j;
                                float v;
                                if (ks < 0) v = k < kx ? dirs[d].w_ih[(size_t)n * kx + k] : 0.0f;
                                else v = dirs[d].w_hh[(size_t)n * HID + 32 * ks + k];
                                pack_put_pieces(dst, lane, j, v, 3);
                            }
        }
}

// k_gemm_x6_stream (rnn_gemm.hip): W [N][K] fp32 row-major, N % 512 == 0, K % 32 == 0, as the fragment stream its eight waves read
// front to back. Wave w owns columns [w N / 8, (w + 1) N / 8) and walks them in blocks of 64; its stream is the slots
// [block][k-step of 32][column tile of 16], every slot three 1 KB pieces x0 | x1 | x2 (pack_put_pieces): [8 waves][N / 512 blocks]
// [K / 32][4][3][64 lanes][8]. lane -> weight row w N / 8 + 64 block + 16 tile + (lane & 15), 8 consecutive K values
// 32 ks + 8 (lane >> 4) + j: the B operand of v_mfma_f32_16x16x32_bf16, as in pack_rec_x6_16.
static inline void pack_gemm6_stream(const float* w, size_t N, size_t K, std::vector<uint16_t>& wp) {
    constexpr size_t SL = 3 * 512;
    const size_t NB = N / 512, KS = K / 32;
    wp.assign(8 * NB * KS * 4 * SL, 0);
    uint16_t* dst = wp.data();
    for (size_t wv = 0; wv < 8; wv++)
        for (size_t b = 0; b < NB; b++)
            for (size_t ks = 0; ks < KS; ks++)
                for (size_t ct = 0; ct < 4; ct++, dst += SL)
                    for (int lane = 0; lane < 64; lane++)
                        for (int j = 0; j < 8; j++) {
                            const size_t n = wv * (N / 8) + 64 * b + 16 * ct + (size_t)(lane & 15), k = 32 * ks + 8 * (size_t)(lane >> 4) + j;
                            pack_put_pieces(dst, lane, j, w[n * K + k], 3);
                        }
}

// GRU weights for k_gru16_bf16: per (direction, wave) 24 slots (ks * 3 + g) * 2 + nt of W_hh and, with kx > 0, 6 slots g * 2 + nt of
// W_ih (features beyond kx zero); lane -> unit 32 w + 16 nt + (lane & 15), values k = 32 ks + 8 (lane >> 4) + j
static inline void pack_gru16_bf16(const pv_rnn_dir* dirs, int kx, std::vector<uint16_t>& wp, std::vector<uint16_t>& wx) {
    const int HID = PV_PACK_GRU_H, NW = 4;
    wp.assign((size_t)2 * NW * 24 * 1024, 0);
    wx.assign(kx ? (size_t)2 * NW * 6 * 1024 : 0, 0);
    for (int d = 0; d < 2; d++)
        for (int w = 0; w < NW; w++)
            for (int g = 0; g < 3; g++)
                for (int nt = 0; nt < 2; nt++) {
                    auto fill = [&](uint16_t* dst, bool xpart, int ks) {
                        for (int lane = 0; lane < 64; lane++)
                            for (int j = 0; j < 8; j++) {
                                const int n = g * HID + 32 * w + 16 * nt + (lane & 15), k = 32 * ks + 8 * (lane >> 4) + j;
                                const float v = xpart ? (k < kx ? dirs[d].w_ih[(size_t)n * kx + k] : 0.0f) : dirs[d].w_hh[(size_t)n * HID + k];
                                pack_put_pieces(dst, lane, j, v);
                            }
                    };
                    for (int ks = 0; ks < 4; ks++) fill(wp.data() + ((size_t)(d * NW + w) * 24 + (ks * 3 + g) * 2 + nt) * 1024, false, ks);
                    if (kx) fill(wx.data() + ((size_t)(d * NW + w) * 6 + g * 2 + nt) * 1024, true, 0);
                }
}

// k_tail_bf16, w[4] = linear_2..5 [512][512]: per wave [layer][k-step][column tile] slots of [hi 1 KB | lo 1 KB]; lane -> column
// 64 wave + 32 tile + (lane & 31), values k = 16 ks + 8 (lane >> 5) + j
static inline void pack_tail_bf16(const float* const* w, std::vector<uint16_t>& wp) {
    constexpr int N = PV_PACK_HEAD_N, KS = N / 16;
    wp.assign((size_t)8 * 4 * KS * 2 * 1024, 0);
    for (int wv = 0; wv < 8; wv++)
        for (int l = 0; l < 4; l++)
            for (int ks = 0; ks < KS; ks++)
                for (int g = 0; g < 2; g++) {
                    uint16_t* dst = wp.data() + ((((size_t)wv * 4 + l) * KS + ks) * 2 + g) * 1024;
                    for (int lane = 0; lane < 64; lane++)
                        for (int j = 0; j < 8; j++) {
                            const int n = 64 * wv + 32 * g + (lane & 31), k = 16 * ks + 8 * (lane >> 5) + j;
                            pack_put_pieces(dst, lane, j, w[l][(size_t)n * N + k]);
                        }
                }
}

// k_tail_x6 (the split-6 chain's 32-row tail), w[4] = linear_2..5 [512][512]: pack_tail_bf16's slot order and lane map with
// slots of three pieces [x0 1 KB | x1 1 KB | x2 1 KB]: 8 waves x 4 layers x 32 k-steps x 2 column tiles x 3 KB = 6.3 MB
static inline void pack_tail_x6(const float* const* w, std::vector<uint16_t>& wp) {
    constexpr int N = PV_PACK_HEAD_N, KS = N / 16;
    constexpr size_t SL = 3 * 512;
    wp.assign((size_t)8 * 4 * KS * 2 * SL, 0);
    for (int wv = 0; wv < 8; wv++)
        for (int l = 0; l < 4; l++)
            for (int ks = 0; ks < KS; ks++)
                for (int g = 0; g < 2; g++) {
                    uint16_t* dst = wp.data() + ((((size_t)wv * 4 + l) * KS + ks) * 2 + g) * SL;
                    for (int lane = 0; lane < 64; lane++)
                        for (int j = 0; j < 8; j++) {
                            const int n = 64 * wv + 32 * g + (lane & 31), k = 16 * ks + 8 * (lane >> 5) + j;
                            pack_put_pieces(dst, lane, j, w[l][(size_t)n * N + k], 3);
                        }
                }
}

// P2's dense layer, dense_w [5][256], as one more MFMA tile of the decoder's steps.
// k_gru16_bf16: [2 dirs][4 waves] slots of [hi 1 KB | lo 1 KB]; wave w of direction d takes k-step w (32 units); lane -> class
// lane & 15 (zero beyond the five), values k = 32 w + 8 (lane >> 4) + j
static inline void pack_p2_dense16(const float* dense_w, std::vector<uint16_t>& f) {
    constexpr int NC = PV_PACK_NCLS, HG = PV_PACK_GRU_H;
    f.assign((size_t)2 * 4 * 1024, 0);
    for (int d = 0; d < 2; d++)
        for (int w = 0; w < 4; w++) {
            uint16_t* dst = f.data() + ((size_t)d * 4 + w) * 1024;
            for (int lane = 0; lane < 64; lane++)
                for (int j = 0; j < 8; j++) {
                    const int n = lane & 15, k = 32 * w + 8 * (lane >> 4) + j;
                    pack_put_pieces(dst, lane, j, n < NC ? dense_w[(size_t)n * 2 * HG + d * HG + k] : 0.0f);
                }
        }
}
// k_rec_bf16: [2 dirs][4 waves][2 k-steps] slots of [hi 1 KB | lo 1 KB]; wave w of direction d takes k-steps 2w, 2w + 1 of that
// direction's 128 units; lane -> class lane & 31 (zero beyond the five), values k = 16 ks + 8 (lane >> 5) + j
static inline void pack_p2_dense(const float* dense_w, std::vector<uint16_t>& f) {
    constexpr int NC = PV_PACK_NCLS, HG = PV_PACK_GRU_H;
    f.assign((size_t)2 * 4 * 2 * 1024, 0);
    for (int d = 0; d < 2; d++)
        for (int w = 0; w < 4; w++)
            for (int kk = 0; kk < 2; kk++) {
                uint16_t* dst = f.data() + (((size_t)d * 4 + w) * 2 + kk) * 1024;
                for (int lane = 0; lane < 64; lane++)
                    for (int j = 0; j < 8; j++) {
                        const int n = lane & 31, k = 16 * (2 * w + kk) + 8 * (lane >> 5) + j;
                        pack_put_pieces(dst, lane, j, n < NC ? dense_w[(size_t)n * 2 * HG + d * HG + k] : 0.0f);
                    }
            }
}
