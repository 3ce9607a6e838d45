// split3_host.hpp — host-only: fp32 -> bf16 pieces as the kernels on the bf16 MFMA make them, for weights that are split once
// at load time (pv_pack_rec_bf16, the planes of k_gemm_bf16x6). No HIP, no other header of the library: the tests compile it
// alone (tests/split3_shim.cpp).
//
// The rule (split3_bf16 in mfma_tiles.hpp is the device form): x0 = rne_bf16(x), x1 = rne_bf16(x - x0),
// x2 = rne_bf16(x - x0 - x1). Both residuals are exact in fp32, so x = x0 + x1 + x2 for every normal x whose third piece is
// not subnormal: three 8-bit significands carry the 24 bits. Two-piece operands (hi, lo) are the first two.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

static inline uint16_t f2bf_bits(float x) {  // round to nearest even
    uint32_t u;
    memcpy(&u, &x, 4);
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
static inline float bf_bits2f(uint16_t h) {
    const uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static inline void split3_bits(float x, uint16_t p[3]) {
    p[0] = f2bf_bits(x);
    const float r1 = x - bf_bits2f(p[0]);
    p[1] = f2bf_bits(r1);
    p[2] = f2bf_bits(r1 - bf_bits2f(p[1]));
}
// w [N][K] fp32 row-major -> three planes [N][K] of bf16 bits: element (n, k) of piece p at p * N * K + n * K + k
static inline void split3_planes(const float* w, size_t N, size_t K, uint16_t* planes) {
    const size_t n = N * K;
    for (size_t i = 0; i < n; i++) {
        uint16_t p[3];
        split3_bits(w[i], p);
        planes[i] = p[0];
        planes[n + i] = p[1];
        planes[2 * n + i] = p[2];
    }
}
