// rust-modem_amd/csrc/modem_frame_math.h — the per-term and per-hit arithmetic of the frame
// synchronizer (include/modem_hip.h, "Frame synchronizer"): one term of the correlation and of the
// energy, the join of the four accumulators, the candidate test, the metric, and the rotation index
// and rotation of the gather. Compiles for the device and for a plain host compiler, as
// modem_sync_math.h does. Every f32 operation is written out (contract off, explicit fma): the
// correlate kernel's tile and halo positions round alike, which is what makes any cut of a stream
// give the same hits.
#pragma once

#include "modem_sync_math.h"

namespace mk {

// One accumulator (cr, ci, e) of the four, and term j of position k: r = r[k + j], u = u[j].
//   cr += r.re u.re + r.im u.im      ci += r.im u.re - r.re u.im      e += r.re^2 + r.im^2
// each as two fused multiply-adds into the accumulator, in the order written.
MODEM_CHAN_HD void frame_mac(float& cr, float& ci, float& e, float rr, float ri, float ur, float ui) {
#pragma clang fp contract(off)
    cr = __builtin_fmaf(rr, ur, cr);
    cr = __builtin_fmaf(ri, ui, cr);
    ci = __builtin_fmaf(ri, ur, ci);
    ci = __builtin_fmaf(-rr, ui, ci);
    e = __builtin_fmaf(rr, rr, e);
    e = __builtin_fmaf(ri, ri, e);
}

MODEM_CHAN_HD float frame_join(const float (&a)[4]) {
#pragma clang fp contract(off)
    return (a[0] + a[1]) + (a[2] + a[3]);
}

// m = |c|^2
MODEM_CHAN_HD float frame_mag(float cr, float ci) {
#pragma clang fp contract(off)
    return __builtin_fmaf(cr, cr, ci * ci);
}

MODEM_CHAN_HD bool frame_finite(float v) { return __builtin_fabsf(v) < __builtin_inff(); }

// pass[k]: m and e finite, m > 0, m >= t2 * e
MODEM_CHAN_HD bool frame_pass(float m, float e, float t2) {
#pragma clang fp contract(off)
    return frame_finite(m) && frame_finite(e) && m > 0.0f && m >= t2 * e;
}

// sqrt(m / (e * Eu)) of a hit (m > 0, so e > 0)
MODEM_CHAN_HD float frame_metric(float m, float e, float eu) {
#pragma clang fp contract(off)
    const float q = m / (e * eu);
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_sqrtf(q);
#else
    return sqrtf(q);
#endif
}

// The multiple of 1 / M turn nearest to phi (M = 2^lm, lm = 1..3), wrapping: 0 .. M-1.
MODEM_CHAN_HD uint32_t frame_rot(uint32_t phi, int lm) { return (uint32_t)(phi + (1u << (31 - lm))) >> (32 - lm); }

// (re, im) e^{-j 2 pi rot / M}: swaps and sign changes for the multiples of a quarter turn (exact),
// a product in f32 by chan_sincos_turn(rot << 29) for the odd eighths of M = 8.
MODEM_CHAN_HD void frame_rotate(float& re, float& im, uint32_t rot, int lm) {
#pragma clang fp contract(off)
    const uint32_t e8 = lm ? rot << (3 - lm) : 0;           // in eighths of a turn
    float a = re, b = im;
    if (e8 & 1) {
        float c, s;
        chan_sincos_turn(e8 << 29, c, s);
        a = __builtin_fmaf(im, s, re * c);
        b = __builtin_fmaf(-re, s, im * c);
    } else {
        switch (e8 >> 1) {
        case 1: a = im; b = -re; break;
        case 2: a = -re; b = -im; break;
        case 3: a = -im; b = re; break;
        default: break;
        }
    }
    re = a;
    im = b;
}

}  // namespace mk
