// Test shim: pack_tail_x6 of pepper_thesis_amd/csrc/rnn_pack_host.hpp behind a C ABI, compiled with the system C++ compiler (no
// HIP) and called through ctypes by tests/test_tail_x6_pack_cpu.py. Same conventions as tests/rnn_pack_x6_shim.cpp: the weights
// arrive as one array over the four layers (w [4][512][512], linear_2..5); the packer returns the number of elements it made
// and copies at most `cap` of them to `out`.
#include "../pepper_thesis_amd/csrc/rnn_pack_host.hpp"

#include <algorithm>

extern "C" {
// out[3 * i + p]: the bits of piece p of x[i]
void shim_split3(const float* x, int64_t n, uint16_t* out) {
    for (int64_t i = 0; i < n; i++) split3_bits(x[i], out + 3 * i);
}
int64_t shim_pack_tail_x6(const float* w, uint16_t* wp, int64_t cap) {
    constexpr int64_t N = PV_PACK_HEAD_N;
    const float* layers[4] = {w, w + N * N, w + 2 * N * N, w + 3 * N * N};
    std::vector<uint16_t> v;
    pack_tail_x6(layers, v);
    std::copy(v.begin(), v.begin() + std::min<int64_t>(cap, (int64_t)v.size()), wp);
    return (int64_t)v.size();
}
}
