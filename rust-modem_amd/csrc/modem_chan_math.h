// rust-modem_amd/csrc/modem_chan_math.h — the per-sample arithmetic of the channel model
// (include/modem_hip.h, "Channel model"): the splitmix64 finaliser, sin/cos of an exact binary
// fraction of a turn, the unit-variance complex Gaussian of a 64-bit word and the sample update.
// Compiles for the device and for a plain host compiler (as modem_scan_step.h does), so that the
// same text can be checked against double on the CPU; on the host log2f / sqrtf stand in for
// v_log_f32 / v_sqrt_f32. Every f32 operation is written out (contract off, explicit fma): the
// wide, narrow and tail paths of the kernel and all its specialisations round alike, which is
// what makes any cut of a stream give the same bytes.
#pragma once

#include <cstdint>
#if !defined(__HIPCC__)
#include <cmath>
#endif

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MODEM_CHAN_HD __host__ __device__ __forceinline__
#else
#define MODEM_CHAN_HD inline
#endif

namespace mk {

constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ULL;

// splitmix64's finaliser (prng_bits, modem_misc.hip)
MODEM_CHAN_HD uint64_t chan_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// cos and sin of 2 pi P / 2^32. The quarter turn nearest to P is split off in integers (exact),
// the remainder f in [-1/8, 1/8] turns goes through the Cephes sinf / cosf minimax polynomials
// for |a| <= pi/4 with the powers of 2 pi folded into the coefficients (a = 2 pi f is never
// formed, so no reduction by 2 pi and no rounding of the angle beyond (float)d, 2^-25 relative).
// Absolute error of either result <= 1.72 * 2^-24 for every P with the low 8 bits clear (all 2^24
// values of the generator's u2) and over random 32-bit P (checked on the host against double).
MODEM_CHAN_HD void chan_sincos_turn(uint32_t P, float& c, float& s) {
#pragma clang fp contract(off)
    constexpr double T = 6.283185307179586476925286766559;
    constexpr float S0 = (float)T, S1 = (float)(-1.6666654611e-1 * T * T * T),
                    S2 = (float)(8.3321608736e-3 * T * T * T * T * T),
                    S3 = (float)(-1.9515295891e-4 * T * T * T * T * T * T * T);
    constexpr float C1 = (float)(-0.5 * T * T), C2 = (float)(4.166664568298827e-2 * T * T * T * T),
                    C3 = (float)(-1.388731625493765e-3 * T * T * T * T * T * T),
                    C4 = (float)(2.443315711809948e-5 * T * T * T * T * T * T * T * T);
    const uint32_t k = (P + 0x20000000u) >> 30;
    const int32_t d = (int32_t)(P - (k << 30));                 // [-2^29, 2^29)
    const float f = (float)d * 0x1p-32f;
    const float z = f * f;
    float ps = __builtin_fmaf(z, S3, S2);
    ps = __builtin_fmaf(z, ps, S1);
    ps = __builtin_fmaf(z, ps, S0);
    const float sn = f * ps;
    float pc = __builtin_fmaf(z, C4, C3);
    pc = __builtin_fmaf(z, pc, C2);
    pc = __builtin_fmaf(z, pc, C1);
    const float cs = __builtin_fmaf(z, pc, 1.0f);
    // rotate by k quarter turns
    const float a = (k & 1) ? sn : cs, b = (k & 1) ? cs : sn;   // k odd: cos = -+sin, sin = +-cos
    c = ((k + 1) & 2) ? -a : a;                                  // k = 1, 2: negative
    s = (k & 2) ? -b : b;                                        // k = 2, 3: negative
}

// w of the word: sqrt(-ln u1) * (cos, sin)(2 pi u2); *r = sqrt(-ln u1).
MODEM_CHAN_HD void chan_gauss(uint64_t word, float& r, float& c, float& s) {
#pragma clang fp contract(off)
    const float u1 = (float)((uint32_t)(word >> 40) + 1u) * 0x1p-24f;     // (0, 1], exact
#if defined(__HIP_DEVICE_COMPILE__)
    const float l2 = __builtin_amdgcn_logf(u1);                           // v_log_f32: u1 is normal
    r = __builtin_amdgcn_sqrtf(l2 * -0x1.62e43p-1f);                      // -ln 2
#else
    r = sqrtf(log2f(u1) * -0x1.62e43p-1f);
#endif
    chan_sincos_turn((uint32_t)word & 0xffffff00u, c, s);                 // u2 = 24 bits of a turn
}

// y = gain * x * e^{j theta} + sig * w. cnt = k + (n + 1) * GOLDEN, ph = phase0 + step * n.
template <bool NOISE, bool ROT>
MODEM_CHAN_HD void chan_sample(float& re, float& im, uint64_t cnt, uint64_t ph, float gain, float sig) {
#pragma clang fp contract(off)
    float yr, yi;
    if (ROT) {
        float c, s;
        chan_sincos_turn((uint32_t)(ph >> 32), c, s);
        const float gc = gain * c, gs = gain * s;
        yr = __builtin_fmaf(-im, gs, re * gc);
        yi = __builtin_fmaf(im, gc, re * gs);
    } else {
        yr = gain * re;
        yi = gain * im;
    }
    if (NOISE) {
        float r, c, s;
        chan_gauss(chan_mix(cnt), r, c, s);
        const float a = sig * r;
        yr = __builtin_fmaf(a, c, yr);
        yi = __builtin_fmaf(a, s, yi);
    }
    re = yr;
    im = yi;
}

}  // namespace mk
