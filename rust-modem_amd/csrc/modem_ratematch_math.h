// rust-modem_amd/csrc/modem_ratematch_math.h — the integer rules of rate matching and of the frame
// check that must agree everywhere (include/modem_hip.h, "Rate matching and frame check"): the rank
// of a kept mother index, the number of kept indices, the pruned block interleaver, and the CRC: its
// bit step, the multiplication of two registers modulo the polynomial, and the split of a row into
// the 64 chunks whose partial registers a wave combines. Compiles for the device and for a plain
// host compiler, as modem_fec_math.h does: the kernels of modem_ratematch.hip, the argument checks
// of capi_ratematch.cpp and the host program of tests/cpp/ratematch_host.cpp all read this text.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MODEM_RM_HD __host__ __device__ __forceinline__
#else
#define MODEM_RM_HD inline
#endif

namespace mk {

constexpr int kRmMaxP = 64;                    // pattern length: the pattern is one 64-bit mask
constexpr int kRmMaxCols = 256;
constexpr int kRmMaxNm = 16384;                // mother indices of a frame
constexpr int kCrcMaxBits = 65536;             // message bits of a row
constexpr int kCrcChunks = 64;                 // a lane of the wave each

MODEM_RM_HD uint32_t rm_popcount(uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popcll(v);
#else
    return (uint32_t)__builtin_popcountll(v);
#endif
}

// The pattern as a mask: bit i is pattern[i], i < P. #{i < c : pattern[i] = 1}, 0 <= c <= P <= 64.
MODEM_RM_HD uint32_t rm_prefix(uint64_t mask, uint32_t c) { return c >= 64 ? rm_popcount(mask) : rm_popcount(mask & (((uint64_t)1 << c) - 1)); }

MODEM_RM_HD bool rm_is_kept(uint64_t mask, uint32_t P, uint32_t m) { return (mask >> (m % P)) & 1u; }

// Rank of mother index m among the kept ones (meaningful for a kept m); w the pattern's weight.
MODEM_RM_HD uint32_t rm_rank(uint64_t mask, uint32_t P, uint32_t w, uint32_t m) {
    const uint32_t r = m / P;
    return r * w + rm_prefix(mask, m - r * P);
}

// E: the kept indices below nm.
MODEM_RM_HD uint32_t rm_kept(uint64_t mask, uint32_t P, uint32_t nm) {
    const uint32_t r = nm / P;
    return r * rm_popcount(mask) + rm_prefix(mask, nm - r * P);
}

MODEM_RM_HD uint32_t rm_rows(uint32_t E, uint32_t C) { return (E + C - 1) / C; }

// The pruned block interleaver: input j of E, written by rows of C, read by columns, the absent
// cells of the last row (columns cl and up, cl = E - (rows - 1) C) skipped.
MODEM_RM_HD uint32_t rm_pi(uint32_t j, uint32_t C, uint32_t rows, uint32_t cl) {
    const uint32_t r = j / C, c = j - r * C;
    return c * rows + r - (c > cl ? c - cl : 0u);
}

// ---- CRC: W in {8, 16, 24, 32}, the register in the low W bits of a uint32_t ----
MODEM_RM_HD uint32_t crc_mask(uint32_t W) { return 0xFFFFFFFFu >> (32u - W); }

// One message bit b (only bit 0 counts).
MODEM_RM_HD uint32_t crc_step(uint32_t reg, uint32_t b, uint32_t W, uint32_t poly) {
    const uint32_t fb = ((reg >> (W - 1)) ^ b) & 1u;
    reg = (reg << 1) & crc_mask(W);
    return fb ? reg ^ poly : reg;
}

// a * b modulo the polynomial, registers read as polynomials over GF(2) of degree < W: W steps, a
// multiplication by x (a step with a zero bit) and an addition of a each.
MODEM_RM_HD uint32_t crc_mul(uint32_t a, uint32_t b, uint32_t W, uint32_t poly) {
    uint32_t r = 0;
    for (int i = (int)W - 1; i >= 0; --i) {
        r = crc_step(r, 0u, W, poly);
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}

// x^n modulo the polynomial.
MODEM_RM_HD uint32_t crc_xpow(uint32_t n, uint32_t W, uint32_t poly) {
    uint32_t r = 1;
    for (uint32_t i = 0; i < n; ++i) r = crc_step(r, 0u, W, poly);
    return r;
}

// The chunks of a row of L >= 1 bits: all of len = ceil(L / 64) bits and aligned to the end of the
// row, so that (63 - l) len bits follow chunk l; the first chunks are cut at bit 0 or empty.
MODEM_RM_HD uint32_t crc_chunk_len(uint32_t L) { return (L + kCrcChunks - 1) / kCrcChunks; }
MODEM_RM_HD void crc_chunk(uint32_t L, uint32_t l, uint32_t& begin, uint32_t& end) {
    const uint32_t len = crc_chunk_len(L), after = (kCrcChunks - 1 - l) * len;
    end = L > after ? L - after : 0u;
    begin = end > len ? end - len : 0u;
}

// The register of chunk l: the bit steps over its bits, from `init` where the chunk holds bit 0 of
// the row (the register of the empty prefix), else from 0 (an empty chunk stays 0). bit(i) returns
// message bit i.
template <typename Bit>
MODEM_RM_HD uint32_t crc_chunk_reg(uint32_t L, uint32_t l, uint32_t W, uint32_t poly, uint32_t init, Bit bit) {
    uint32_t b, e;
    crc_chunk(L, l, b, e);
    uint32_t reg = (b == 0 && e > 0) ? init : 0u;
    for (uint32_t i = b; i < e; ++i) reg = crc_step(reg, (uint32_t)bit(i), W, poly);
    return reg;
}

// Two neighbouring blocks of chunks into one: `left` is followed by the bits of `right`, whose
// number is the exponent of xp = x^bits mod poly.
MODEM_RM_HD uint32_t crc_join(uint32_t left, uint32_t right, uint32_t xp, uint32_t W, uint32_t poly) {
    return crc_mul(left, xp, W, poly) ^ right;
}

}  // namespace mk
