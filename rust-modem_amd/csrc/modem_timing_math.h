// rust-modem_amd/csrc/modem_timing_math.h — the per-block and per-symbol arithmetic of the symbol
// timing synchronizer (include/modem_hip.h, "Symbol timing synchronizer"): the symbol-rate line of
// the N phase energies, the position of an output symbol on a block's line, and the four cubic
// Lagrange coefficients. Compiles for the device and for a plain host compiler, as
// modem_sync_math.h does. Every f32 operation is written out (contract off, explicit fma), so every
// path of the kernels rounds alike.
#pragma once

#include "modem_sync_math.h"

namespace mk {

// S = sum_p E_p and X = sum_p E_p e^{-j 2 pi p / N} for N = 4 (ln = 2) or 8 (ln = 3).
MODEM_CHAN_HD void timing_line(const float (&E)[8], int ln, float& re, float& im, float& S) {
#pragma clang fp contract(off)
    if (ln == 2) {
        S = (E[0] + E[1]) + (E[2] + E[3]);
        re = E[0] - E[2];
        im = E[3] - E[1];
    } else {
        const float h = 0.70710678118654752440f;                 // (float)sqrt(0.5)
        S = ((E[0] + E[1]) + (E[2] + E[3])) + ((E[4] + E[5]) + (E[6] + E[7]));
        const float d0 = E[0] - E[4], d1 = E[1] - E[5], d2 = E[2] - E[6], d3 = E[3] - E[7];
        re = d0 + h * (d1 - d3);
        im = -(d2 + h * (d1 + d3));
    }
}

// Phi = (0 - turn32(X.im, X.re)) mod 2^32
MODEM_CHAN_HD uint32_t timing_phi(float re, float im) { return 0u - sync_atan2_turn(im, re); }

// The position of line offset i (0 .. B-1, or B .. for the flushed rest, whose output offset is
// i - B) of a block with delay D and slope s: Q32.32 samples relative to the first sample of the
// block the output offset counts from. io = the output offset (i, or i - B in the flush).
MODEM_CHAN_HD int64_t timing_pos(int64_t D, int64_t s, int64_t i, int64_t io, int lb, int ln, int span) {
    const int64_t one = (int64_t)1 << 32, lim = span * one;
    int64_t e = D + s * (2 * i - ((int64_t)1 << lb) + 1);
    e = e < -lim ? -lim : e > lim ? lim : e;
    return ((io - span) * one + e) * ((int64_t)1 << ln);
}

// mu of a position: its fraction's top 24 bits, exact in f32
MODEM_CHAN_HD float timing_mu(int64_t Q) { return (float)(((uint64_t)Q & 0xffffffffu) >> 8) * 0x1p-24f; }

// c_-1 .. c_2 of the cubic Lagrange interpolator at mu in [0, 1); mu = 0 gives (-0, 1, 0, -0).
MODEM_CHAN_HD void timing_coefs(float mu, float (&c)[4]) {
#pragma clang fp contract(off)
    const float k6 = 0.16666666666666666667f;                    // (float)(1.0 / 6.0)
    const float a = mu + 1.0f, b = mu - 1.0f, d = mu - 2.0f;
    const float mb = mu * b, am = a * mu;
    c[0] = -(mb * d) * k6;
    c[1] = ((a * b) * d) * 0.5f;
    c[2] = -(am * d) * 0.5f;
    c[3] = (am * b) * k6;
}

// sum_j c_j x_j, j ascending: one product, then three fused multiply-adds
MODEM_CHAN_HD float timing_dot(const float (&c)[4], float x0, float x1, float x2, float x3) {
#pragma clang fp contract(off)
    float acc = c[0] * x0;
    acc = __builtin_fmaf(c[1], x1, acc);
    acc = __builtin_fmaf(c[2], x2, acc);
    acc = __builtin_fmaf(c[3], x3, acc);
    return acc;
}

}  // namespace mk
