// rust-modem_amd/csrc/modem_fec_math.h — the pieces of the convolutional code that must agree
// everywhere (include/modem_hip.h, "Convolutional code"): the parity of a tapped register, the
// encoder step, the quantiser of the decoder's input, the predecessor of a trellis state and the
// branch word of a state (the coded bits of its two incoming branches). Compiles for the device and
// for a plain host compiler, as modem_scan_step.h does: the kernels of modem_fec.hip, the handle's
// table in capi_fec.cpp and the host decoder of tests/cpp/fec_host.cpp all read this text. All of
// it is integer arithmetic but the one f32 product of the quantiser.
#pragma once

#include <cstdint>
#if !defined(__HIPCC__)
#include <cmath>
#endif

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MODEM_FEC_HD __host__ __device__ __forceinline__
#else
#define MODEM_FEC_HD inline
#endif

namespace mk {

constexpr int kFecMinK = 3, kFecMaxK = 9;
constexpr int kFecMaxN = 3;                    // generator polynomials (rate 1/2 and 1/3)
constexpr int kFecDecWords = 4096;             // 64-bit decision words a frame group keeps: 32 KiB
constexpr int32_t kFecStart = -(1 << 30);      // the path metric of every state but 0 at step 0

// Steps a frame may have: T * max(1, S / 64) decision words must fit.
MODEM_FEC_HD int fec_max_steps(int K) { return K <= 7 ? kFecDecWords : kFecDecWords >> (K - 7); }

MODEM_FEC_HD uint32_t fec_parity(uint32_t v) {
    v ^= v >> 16;
    v ^= v >> 8;
    v ^= v >> 4;
    v ^= v >> 2;
    v ^= v >> 1;
    return v & 1u;
}

// Coded bit j of the register reg = (b << (K-1)) | s.
MODEM_FEC_HD uint32_t fec_coded_bit(uint32_t reg, uint32_t g) { return fec_parity(reg & g); }

// The register of step t of a frame: bit K-1-d is information bit t-d (0 before the frame and in
// the tail), so reg = (bit_t << (K-1)) | state. bit(i) returns information bit i, 0 <= i < nbits.
template <typename Bit>
MODEM_FEC_HD uint32_t fec_register(int K, int64_t t, int64_t nbits, Bit bit) {
    uint32_t reg = 0;
    for (int d = 0; d < K; ++d) {
        const int64_t i = t - d;
        if (i >= 0 && i < nbits) reg |= (uint32_t)(bit(i) & 1u) << (K - 1 - d);
    }
    return reg;
}

// Predecessor x of state s' (S = 2^(K-1) states).
MODEM_FEC_HD uint32_t fec_pred(uint32_t sn, uint32_t x, int K) { return ((sn << 1) & ((1u << (K - 1)) - 1u)) | x; }

// The input bit that leads into state s'.
MODEM_FEC_HD uint32_t fec_input_bit(uint32_t sn, int K) { return sn >> (K - 2); }

// Branch word of state s': bit x * kFecMaxN + j is coded bit j on the branch from predecessor x.
MODEM_FEC_HD uint32_t fec_branch_word(uint32_t sn, int K, const uint32_t* g, int n) {
    uint32_t w = 0;
    for (uint32_t x = 0; x < 2; ++x) {
        const uint32_t reg = (fec_input_bit(sn, K) << (K - 1)) | fec_pred(sn, x, K);
        for (int j = 0; j < n; ++j) w |= fec_coded_bit(reg, g[j]) << (x * kFecMaxN + j);
    }
    return w;
}

// 1 - 2 c for bit k of a branch word.
MODEM_FEC_HD int32_t fec_branch_sign(uint32_t w, int k) { return 1 - 2 * (int32_t)((w >> k) & 1u); }

// The quantiser. I8: -128 joins -127. F32 (and F16 widened exactly): one f32 product, clamped to
// +-127, rounded to nearest, ties to even. A NaN is unspecified by the contract; here it gives -127.
MODEM_FEC_HD int32_t fec_quant_i8(int8_t v) { return v < -127 ? -127 : (int32_t)v; }
MODEM_FEC_HD int32_t fec_quant_f32(float v, float qscale) {
#pragma clang fp contract(off)
    const float p = v * qscale;
#if defined(__HIP_DEVICE_COMPILE__)
    return (int32_t)__builtin_rintf(__builtin_fminf(__builtin_fmaxf(p, -127.0f), 127.0f));
#else
    return (int32_t)rintf(fminf(fmaxf(p, -127.0f), 127.0f));
#endif
}

// One add-compare-select: the survivor is predecessor 1 iff m1 > m0 (ties keep 0).
MODEM_FEC_HD int32_t fec_acs(int32_t m0, int32_t m1, uint32_t& x) {
    x = m1 > m0 ? 1u : 0u;
    return x ? m1 : m0;
}

}  // namespace mk
