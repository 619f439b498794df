// rust-modem_amd/csrc/modem_llr_store.h — the LLR output side shared by the soft demapper
// (modem_demap.hip) and the noncoherent detectors (modem_noncoh.hip): a value's output dtype
// rules and a lane's packed stores at the widest width its address allows.
#pragma once

#include "modem_device.h"

namespace mk {

// A lane's BPS outputs as packed 32-bit words (element e at byte e * sizeof(OutT)).
template <typename OutT> struct DemapOut;
template <> struct DemapOut<float> {
    static constexpr int esz = 4;
    static __device__ __forceinline__ uint32_t bits(float v) { return __float_as_uint(v); }
};
template <> struct DemapOut<__half> {   // round to nearest, saturating: never inf
    static constexpr int esz = 2;
    static __device__ __forceinline__ uint32_t bits(float v) {
        const float c = __builtin_fminf(__builtin_fmaxf(v, -65504.f), 65504.f);
        return (uint32_t)__half_as_ushort(__float2half_rn(c));
    }
};
template <> struct DemapOut<int8_t> {   // rint(clamp(v, -127, 127))
    static constexpr int esz = 1;
    static __device__ __forceinline__ uint32_t bits(float v) {
        const float c = __builtin_fminf(__builtin_fmaxf(v, -127.f), 127.f);
        return (uint32_t)(int)__builtin_rintf(c) & 0xffu;
    }
};

typedef uint32_t demap_u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t demap_u32x4 __attribute__((ext_vector_type(4)));

// The lane's B bytes at dst as B / W stores of W bytes (dst is W-aligned, W divides B).
template <int W, int B, int NW>
__device__ __forceinline__ void demap_store(char* dst, const uint32_t (&w)[NW]) {
#pragma unroll
    for (int o = 0; o < B; o += W) {
        if constexpr (W == 16) {
            demap_u32x4 v = {w[o / 4], w[o / 4 + 1], w[o / 4 + 2], w[o / 4 + 3]};
            *reinterpret_cast<demap_u32x4*>(dst + o) = v;
        } else if constexpr (W == 8) {
            demap_u32x2 v = {w[o / 4], w[o / 4 + 1]};
            *reinterpret_cast<demap_u32x2*>(dst + o) = v;
        } else if constexpr (W == 4) {
            *reinterpret_cast<uint32_t*>(dst + o) = w[o / 4];
        } else if constexpr (W == 2) {
            *reinterpret_cast<uint16_t*>(dst + o) = (uint16_t)(w[o / 4] >> (8 * (o % 4)));
        } else {
            *reinterpret_cast<uint8_t*>(dst + o) = (uint8_t)(w[o / 4] >> (8 * (o % 4)));
        }
    }
}

// Bytes per store for a lane's B bytes at `out` + k * B: the largest power of two <= 16 dividing B
// and the base address (wave-uniform).
inline int demap_store_width(const void* out, int B) {
    const uintptr_t low = (reinterpret_cast<uintptr_t>(out) | (uintptr_t)B | 16u);
    return (int)(low & (~low + 1));                         // lowest set bit: 1, 2, 4, 8 or 16
}

// A lane's NB values as NB elements of OutT at dst (= out + k * B), by stores of vw bytes.
template <typename OutT, int NB>
__device__ __forceinline__ void demap_put(char* dst, const float (&v)[NB], int vw) {
    constexpr int ESZ = DemapOut<OutT>::esz, B = NB * ESZ, NW = (B + 3) / 4;
    uint32_t w[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i) w[i] = 0;
#pragma unroll
    for (int j = 0; j < NB; ++j) w[j * ESZ / 4] |= DemapOut<OutT>::bits(v[j]) << (8 * (j * ESZ % 4));
    if constexpr (B % 16 == 0) { if (vw == 16) { demap_store<16, B>(dst, w); return; } }
    if constexpr (B % 8 == 0) { if (vw >= 8) { demap_store<8, B>(dst, w); return; } }
    if constexpr (B % 4 == 0) { if (vw >= 4) { demap_store<4, B>(dst, w); return; } }
    if constexpr (B % 2 == 0) { if (vw >= 2) { demap_store<2, B>(dst, w); return; } }
    if constexpr (ESZ == 1) demap_store<1, B>(dst, w);
}

}  // namespace mk
