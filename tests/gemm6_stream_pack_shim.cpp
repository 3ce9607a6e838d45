// Test shim: pack_gemm6_stream of pepper_thesis_amd/csrc/rnn_pack_host.hpp behind a C ABI, compiled with the system C++ compiler (no
// HIP) and called through ctypes by tests/test_gemm_x6_stream_pack_cpu.py. Same conventions as tests/rnn_pack_x6_shim.cpp: the
// packer returns the number of elements it made and copies at most `cap` of them to `out`.
#include "../pepper_thesis_amd/csrc/rnn_pack_host.hpp"

#include <algorithm>

extern "C" {
// out[3 * i + p]: the bits of piece p of x[i]
void shim_split3(const float* x, int64_t n, uint16_t* out) {
    for (int64_t i = 0; i < n; i++) split3_bits(x[i], out + 3 * i);
}
int64_t shim_pack_gemm6_stream(const float* w, int64_t N, int64_t K, uint16_t* wp, int64_t cap) {
    std::vector<uint16_t> v;
    pack_gemm6_stream(w, (size_t)N, (size_t)K, v);
    std::copy(v.begin(), v.begin() + std::min<int64_t>(cap, (int64_t)v.size()), wp);
    return (int64_t)v.size();
}
}
