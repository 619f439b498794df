// rust-modem_amd/csrc/modem_sync_math.h — the per-symbol and per-block arithmetic of the carrier
// synchronizer (include/modem_hip.h, "Carrier synchronizer"): the M-th power by repeated complex
// squaring, the angle of a block sum as a 32-bit fraction of a turn, the block quality and the
// derotation. Compiles for the device and for a plain host compiler, as modem_chan_math.h does, so
// that the same text can be checked against double on the CPU (tools/sync_math_check.cpp). Every
// f32 operation is written out (contract off, explicit fma): every path of the kernels rounds
// alike, which is what makes any cut of a stream give the same bytes.
#pragma once

#include "modem_chan_math.h"

namespace mk {

// z = (nrm * (re, im))^(2^lm), lm = 1..3, and mag = |z| = (|nrm r|^2)^(2^(lm-1)) (no square root).
MODEM_CHAN_HD void sync_power(float re, float im, float nrm, int lm, float& zr, float& zi, float& mag) {
#pragma clang fp contract(off)
    float a = nrm * re, b = nrm * im;
    float m = __builtin_fmaf(a, a, b * b);
    for (int j = 0; j < lm; ++j) {
        const float bb = b * b, ab = a * b;
        a = __builtin_fmaf(a, a, -bb);
        b = ab + ab;
        if (j) m = m * m;
    }
    zr = a;
    zi = b;
    mag = m;
}

// The angle of (x, y) as a fraction of a turn, 32 bits: |result / 2^32 - atan2(y, x) / (2 pi)| <=
// 2^-22 (mod 1) for all finite inputs; (0, 0) and non-finite inputs give 0. The octant is split off
// in exact operations (absolute values, a swap, integer reflections); the one rounded quotient
// t = min / max in [0, 1] goes through atan(t) / (2 pi) = t Q(t^2), Q a degree-7 minimax
// polynomial (2^-27.3 turns in exact arithmetic, 2^-25 evaluated in f32).
MODEM_CHAN_HD uint32_t sync_atan2_turn(float y, float x) {
#pragma clang fp contract(off)
    constexpr float Q0 = 1.59154837338999294e-01f, Q1 = -5.30461206953653369e-02f, Q2 = 3.17459422206438635e-02f,
                    Q3 = -2.21362568624719792e-02f, Q4 = 1.53459973410878855e-02f, Q5 = -8.89867488397865641e-03f,
                    Q6 = 3.47956519737998085e-03f, Q7 = -6.45295620257025151e-04f;
    const float ax = __builtin_fabsf(x), ay = __builtin_fabsf(y);
    const bool swap = ay > ax;
    const float num = swap ? ax : ay, den = swap ? ay : ax;
    if (!(den > 0.0f) || !(den < __builtin_inff()) || !(num <= den)) return 0;   // (0, 0), an infinity or a NaN
    const float t = num / den;
    const float z = t * t;
    float p = __builtin_fmaf(z, Q7, Q6);
    p = __builtin_fmaf(z, p, Q5);
    p = __builtin_fmaf(z, p, Q4);
    p = __builtin_fmaf(z, p, Q3);
    p = __builtin_fmaf(z, p, Q2);
    p = __builtin_fmaf(z, p, Q1);
    p = __builtin_fmaf(z, p, Q0);
    uint32_t a = (uint32_t)((t * p) * 0x1p32f);                     // [0, 2^29 + a few]: truncation, 2^-32 turns
    if (swap) a = 0x40000000u - a;
    if (x < 0.0f) a = 0x80000000u - a;
    if (y < 0.0f) a = 0u - a;
    return a;
}

// q = |P| / S; 0 when S is 0 or anything is not finite. |P| is formed from the larger
// component, so neither tiny nor huge sums leave the f32 range on the way.
MODEM_CHAN_HD float sync_quality(float pr, float pi, float S) {
#pragma clang fp contract(off)
    const float ar = __builtin_fabsf(pr), ai = __builtin_fabsf(pi);
    const float hi = ar > ai ? ar : ai, lo = ar > ai ? ai : ar;
    if (!(S > 0.0f) || !(S < __builtin_inff()) || !(hi < __builtin_inff())) return 0.0f;
    if (hi == 0.0f) return 0.0f;
    const float r = lo / hi;
#if defined(__HIP_DEVICE_COMPILE__)
    const float h = hi * __builtin_amdgcn_sqrtf(__builtin_fmaf(r, r, 1.0f));
#else
    const float h = hi * sqrtf(__builtin_fmaf(r, r, 1.0f));
#endif
    return h / S;
}

// The phase of offset i (0 .. B-1, or B .. 2B-1 for the flushed rest) on the line of one block:
// theta + s (2 i - B + 1) mod 2^64.
MODEM_CHAN_HD uint64_t sync_line(uint64_t theta, int64_t s, int64_t i, int64_t B) {
    return theta + (uint64_t)s * (uint64_t)(2 * i - B + 1);
}

// out = r e^{-j 2 pi ph / 2^64}, from the top 32 bits of ph.
MODEM_CHAN_HD void sync_derotate(float& re, float& im, uint64_t ph) {
#pragma clang fp contract(off)
    float c, s;
    chan_sincos_turn((uint32_t)(ph >> 32), c, s);
    const float yr = __builtin_fmaf(im, s, re * c);
    const float yi = __builtin_fmaf(-re, s, im * c);
    re = yr;
    im = yi;
}

}  // namespace mk
