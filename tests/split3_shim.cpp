// Test shim: the piece rule of pepper_thesis_amd/csrc/split3_host.hpp behind a C ABI, compiled with the system C++ compiler
// (no HIP) and called through ctypes by tests/test_split3_host_cpu.py.
#include "../pepper_thesis_amd/csrc/split3_host.hpp"

extern "C" {
// out[3 * i + p]: the bits of piece p of x[i]
void shim_split3(const float* x, int64_t n, uint16_t* out) {
    for (int64_t i = 0; i < n; i++) split3_bits(x[i], out + 3 * i);
}
// planes[3][N][K] from w[N][K]
void shim_split3_planes(const float* w, int64_t N, int64_t K, uint16_t* planes) { split3_planes(w, (size_t)N, (size_t)K, planes); }
}
