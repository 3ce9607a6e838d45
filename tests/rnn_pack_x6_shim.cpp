// Test shim: pack_rec_x6_16 of pepper_thesis_amd/csrc/rnn_pack_host.hpp behind a C ABI, compiled with the system C++ compiler (no
// HIP) and called through ctypes by tests/test_rec_x6_mfma16_pack_cpu.py. Same conventions as tests/rnn_pack_shim.cpp: weights
// arrive as arrays over both directions (w_ih [2][1024][kx] or NULL when kx == 0, w_hh [2][1024][256]); the packer returns the
// number of elements it made and copies at most `cap` of them to `out`.
#include "../pepper_thesis_amd/csrc/rnn_pack_host.hpp"

#include <algorithm>

extern "C" {
// out[3 * i + p]: the bits of piece p of x[i]
void shim_split3(const float* x, int64_t n, uint16_t* out) {
    for (int64_t i = 0; i < n; i++) split3_bits(x[i], out + 3 * i);
}
int64_t shim_pack_rec_x6_16(const float* w_ih, const float* w_hh, int kx, uint16_t* wp, int64_t cap) {
    constexpr int64_t ROWS = 4 * PV_PACK_LSTM_H;
    pv_rnn_dir d[2];
    for (int i = 0; i < 2; i++) d[i] = {w_ih ? w_ih + i * ROWS * kx : nullptr, w_hh + i * ROWS * PV_PACK_LSTM_H, nullptr, nullptr};
    std::vector<uint16_t> v;
    pack_rec_x6_16(d, kx, v);
    std::copy(v.begin(), v.begin() + std::min<int64_t>(cap, (int64_t)v.size()), wp);
    return (int64_t)v.size();
}
}
