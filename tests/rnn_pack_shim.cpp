// Test shim: the weight packers of pepper_thesis_amd/csrc/rnn_pack_host.hpp behind a C ABI, compiled with the system C++ compiler
// (no HIP) and called through ctypes by tests/test_rnn_pack_host_cpu.py.
//
// Recurrent weights arrive as four arrays over both directions: w_ih [2][G*H][K], w_hh [2][G*H][H], b_ih, b_hh [2][G*H]. Every
// packer returns the number of elements it made and copies at most `cap` of them to `out`; the test sizes `out` from the
// documented layout and checks the count.
#include "../pepper_thesis_amd/csrc/rnn_pack_host.hpp"

#include <algorithm>

namespace {
struct Dirs {
    pv_rnn_dir d[2];
    Dirs(const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int64_t rows, int64_t K, int64_t H) {
        for (int i = 0; i < 2; i++) d[i] = {w_ih ? w_ih + i * rows * K : nullptr, w_hh + i * rows * H, b_ih + i * rows, b_hh + i * rows};
    }
};
template <typename T> int64_t give(const std::vector<T>& v, T* out, int64_t cap) {
    std::copy(v.begin(), v.begin() + std::min<int64_t>(cap, (int64_t)v.size()), out);
    return (int64_t)v.size();
}
}  // namespace

extern "C" {
// out[3 * i + p]: the bits of piece p of x[i]
void shim_split3(const float* x, int64_t n, uint16_t* out) {
    for (int64_t i = 0; i < n; i++) split3_bits(x[i], out + 3 * i);
}
int64_t shim_split8_rows(const float* w, int64_t N, int64_t K, uint16_t* out, int64_t cap) {
    std::vector<uint16_t> v;
    split8_rows(w, (size_t)N, (size_t)K, v);
    return give(v, out, cap);
}
int64_t shim_pack_lstm(const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int K, int KP, int TR, float* wp, int64_t cap,
                       float* bias, int64_t bias_cap, int64_t* n_bias) {
    Dirs dirs(w_ih, w_hh, b_ih, b_hh, 4 * PV_PACK_LSTM_H, K, PV_PACK_LSTM_H);
    std::vector<float> v, b;
    pack_lstm(dirs.d, K, KP, TR, v, b);
    *n_bias = give(b, bias, bias_cap);
    return give(v, wp, cap);
}
int64_t shim_pack_lstm_split(const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int K, int KP, int parts, float* wp,
                             int64_t cap) {
    Dirs dirs(w_ih, w_hh, b_ih, b_hh, 4 * PV_PACK_LSTM_H, K, PV_PACK_LSTM_H);
    std::vector<float> v;
    pack_lstm_split(dirs.d, K, KP, parts, v);
    return give(v, wp, cap);
}
int64_t shim_pack_linear(const float* W, int K, int TR, float* wp, int64_t cap) {
    std::vector<float> v;
    pack_linear(W, K, TR, v);
    return give(v, wp, cap);
}
int64_t shim_pack_gru(const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int K, int KP, int TR, int hx_order, float* wp,
                      int64_t cap, float* bias, int64_t bias_cap, int64_t* n_bias) {
    Dirs dirs(w_ih, w_hh, b_ih, b_hh, 3 * PV_PACK_GRU_H, K, PV_PACK_GRU_H);
    std::vector<float> v, b;
    pack_gru(dirs.d, K, KP, TR, v, b, hx_order != 0);
    *n_bias = give(b, bias, bias_cap);
    return give(v, wp, cap);
}
int64_t shim_pack_gru_us(const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int K, int KP, float* wp, int64_t cap) {
    Dirs dirs(w_ih, w_hh, b_ih, b_hh, 3 * PV_PACK_GRU_H, K, PV_PACK_GRU_H);
    std::vector<float> v;
    pack_gru_us(dirs.d, K, KP, v);
    return give(v, wp, cap);
}
// w_ih may be NULL when kx == 0 (no x-part)
int64_t shim_pack_rec_bf16(const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int cell, int kx, int pieces, uint16_t* wp,
                           int64_t cap, uint16_t* wx, int64_t wx_cap, int64_t* n_wx) {
    const int H = cell == 4 ? PV_PACK_LSTM_H : PV_PACK_GRU_H;
    Dirs dirs(w_ih, w_hh, b_ih, b_hh, cell * H, kx, H);
    std::vector<uint16_t> v, x;
    pack_rec_bf16(dirs.d, cell, kx, pieces, v, x);
    *n_wx = give(x, wx, wx_cap);
    return give(v, wp, cap);
}
int64_t shim_pack_gru16_bf16(const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int kx, uint16_t* wp, int64_t cap,
                             uint16_t* wx, int64_t wx_cap, int64_t* n_wx) {
    Dirs dirs(w_ih, w_hh, b_ih, b_hh, 3 * PV_PACK_GRU_H, kx, PV_PACK_GRU_H);
    std::vector<uint16_t> v, x;
    pack_gru16_bf16(dirs.d, kx, v, x);
    *n_wx = give(x, wx, wx_cap);
    return give(v, wp, cap);
}
// w [4][512][512]: linear_2..5
int64_t shim_pack_tail_bf16(const float* w, uint16_t* wp, int64_t cap) {
    const size_t nn = (size_t)PV_PACK_HEAD_N * PV_PACK_HEAD_N;
    const float* ws[4] = {w, w + nn, w + 2 * nn, w + 3 * nn};
    std::vector<uint16_t> v;
    pack_tail_bf16(ws, v);
    return give(v, wp, cap);
}
int64_t shim_pack_p2_dense(const float* dense_w, int rows16, uint16_t* f, int64_t cap) {
    std::vector<uint16_t> v;
    if (rows16) pack_p2_dense16(dense_w, v);
    else pack_p2_dense(dense_w, v);
    return give(v, f, cap);
}
}
