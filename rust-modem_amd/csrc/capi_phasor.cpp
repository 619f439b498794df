// rust-modem_amd/csrc/capi_phasor.cpp — C ABI, host side: status strings, freq / rates / PLL,
// carrier phases, the phasor LUT builders (the memoryless DigitalPhasor plugins evaluated once per
// symbol value, same expressions and rounding as the reference), the slicer and the RRC taps.
#include "capi_common.h"

#include <cmath>
#include <cstring>

#pragma clang fp contract(off)

using namespace capi;

namespace {

// ---- reference restatements used by the LUT builder (digital/util.rs, util.rs) ----------
float bit_to_sign(uint8_t b) { return (float)(int8_t)(2 * (int8_t)b - 1); }   // digital/util.rs:1-3
uint8_t bytes_to_bits(const uint8_t* b, size_t n) {                            // digital/util.rs:5-11
    if (n == 0) return 0;
    uint8_t s = 0;
    for (size_t i = 0; i < n; ++i) s = (uint8_t)(s | (uint8_t)((b[i] & 1) << (n - 1 - i)));
    return s;
}
float mod_trig(float x) {                                                      // util.rs:3-6
    const float two_pi = kPi * 2.0f;
    return x - two_pi * std::floor(x / two_pi);
}

// i(_, b), q(_, b) of one memoryless phasor for the bit slice b (MSB first).
modem_status phasor_iq(const modem_phasor_desc* d, const uint8_t* b, size_t n, float* i, float* q) {
    const float A = d->amplitude;
    switch (d->kind) {
    case MODEM_PHASOR_BPSK: {                                     // bpsk.rs:17-31
        const float c = bit_to_sign(b[0]) * A;
        *i = c * std::cos(d->phase); *q = c * std::sin(d->phase);
        return MODEM_OK;
    }
    case MODEM_PHASOR_QPSK: {                                     // qpsk.rs:11-35
        const float pc = std::cos(d->phase), ps = std::sin(d->phase);
        const float amp = A * std::sqrt(0.5f);
        *i = amp * (bit_to_sign(b[0]) * pc - bit_to_sign(b[1]) * ps);
        *q = amp * (bit_to_sign(b[1]) * pc + bit_to_sign(b[0]) * ps);
        return MODEM_OK;
    }
    case MODEM_PHASOR_QAM: {                                      // qam.rs:15-60
        const size_t cs = n / 2;
        const float ms = (float)((1u << cs) - 1);
        const float pc = std::cos(d->phase), ps = std::sin(d->phase);
        const float amp = A / ms / 2.0f;
        const float pm = 2.0f * (float)bytes_to_bits(b, cs) - ms;
        const float pl = 2.0f * (float)bytes_to_bits(b + cs, n - cs) - ms;
        *i = amp * (pm * pc - pl * ps);
        *q = amp * (pl * pc + pm * ps);
        return MODEM_OK;
    }
    case MODEM_PHASOR_BASK:                                       // bask.rs:15-24
        *i = (float)b[0] * A; *q = 0.0f;
        return MODEM_OK;
    case MODEM_PHASOR_MPSK: {                                     // mpsk.rs:14-41
        const float ns = (float)(1u << n);
        const float inner = 2.0f * kPi * (float)bytes_to_bits(b, n) / ns + d->phase;
        *i = A * std::cos(inner); *q = A * std::sin(inner);
        return MODEM_OK;
    }
    case MODEM_PHASOR_APSK: {                                     // apsk.rs:36-56
        const uint8_t s = bytes_to_bits(b, n);
        const modem_ring* ring = nullptr;
        for (uint32_t k = 0; k < d->nrings; ++k)
            if (s >= d->rings[k].start && s < d->rings[k].end) { ring = &d->rings[k]; break; }
        if (!ring) return MODEM_ERR_INVALID_ARG;
        const float inner = 2.0f * kPi * (float)(uint8_t)(s - ring->start) /
                            (float)(uint8_t)(ring->end - ring->start) + ring->phase;
        *i = A * ring->radius * std::cos(inner); *q = A * ring->radius * std::sin(inner);
        return MODEM_OK;
    }
    case MODEM_PHASOR_OQPSK: {                                    // oqpsk.rs:9-25
        const float amp = A * std::sqrt(0.5f);
        *i = bit_to_sign(b[0]) * amp; *q = bit_to_sign(b[1]) * amp;
        return MODEM_OK;
    }
    default: return MODEM_ERR_INVALID_ARG;
    }
}

modem_status apsk_verify(const modem_phasor_desc* d, uint32_t bps) {   // apsk.rs:25-26,74,85-97
    if (d->nrings == 0 || !d->rings) return MODEM_ERR_INVALID_ARG;
    unsigned prev = 0;
    for (uint32_t k = 0; k < d->nrings; ++k) {
        const modem_ring& r = d->rings[k];
        if (!(r.radius >= 0.0f && r.radius <= 1.0f)) return MODEM_ERR_INVALID_ARG;
        if (r.start != prev) return MODEM_ERR_INVALID_ARG;
        prev = r.end;
    }
    return prev == (1u << bps) ? MODEM_OK : MODEM_ERR_INVALID_ARG;
}

}  // namespace

modem_status capi::phasor_bps(const modem_phasor_desc* d, uint32_t* bps) {
    switch (d->kind) {
    case MODEM_PHASOR_BPSK: case MODEM_PHASOR_BASK: *bps = 1; return MODEM_OK;
    case MODEM_PHASOR_QPSK: case MODEM_PHASOR_OQPSK: *bps = 2; return MODEM_OK;
    case MODEM_PHASOR_QAM:
        if (d->bits_per_symbol < 2 || d->bits_per_symbol > 8) return MODEM_ERR_INVALID_ARG;  // qam.rs:17
        *bps = d->bits_per_symbol; return MODEM_OK;
    case MODEM_PHASOR_MPSK: case MODEM_PHASOR_APSK: case MODEM_PHASOR_CPFSK: case MODEM_PHASOR_DMPSK:
    case MODEM_PHASOR_MFSK:
        if (d->bits_per_symbol < 1 || d->bits_per_symbol > 8) return MODEM_ERR_INVALID_ARG;
        *bps = d->bits_per_symbol; return MODEM_OK;
    case MODEM_PHASOR_DCQPSK: case MODEM_PHASOR_MSK: *bps = 2; return MODEM_OK;   // dcqpsk.rs:39, msk.rs:28
    case MODEM_PHASOR_BFSK: *bps = 1; return MODEM_OK;                            // bfsk.rs:23
    default: return MODEM_ERR_INVALID_ARG;
    }
}

extern "C" {

const char* modem_status_str(modem_status s) {
    switch (s) {
    case MODEM_OK: return "ok";
    case MODEM_ERR_INVALID_ARG: return "invalid argument (the reference would panic)";
    case MODEM_ERR_UNSUPPORTED: return "unsupported by this backend";
    case MODEM_ERR_HIP: return "HIP runtime error";
    case MODEM_ERR_NO_DEVICE: return "no such HIP device";
    case MODEM_ERR_CAPACITY: return "output buffer too small";
    case MODEM_ERR_ALLOC: return "allocation failed";
    }
    return "unknown status";
}

float modem_freq_sample_freq(uint64_t hz, uint64_t sr) {           // freq.rs:19-26
    const float ang = 2.0f * kPi * (float)hz;
    return ang / (float)sr;
}

modem_status modem_pll_lock(float w, uint64_t s0, const float* x, size_t n, float* off) {
    if (!off || (n && !x)) return MODEM_ERR_INVALID_ARG;
    const float change = 0.447214f;                                          // pll.rs:3
    for (size_t k = 0; k < n; ++k) {                                         // demodulator.rs:33-35
        const float inner = mod_trig(w * (float)(s0 + k)) + *off;            // pll.rs:17
        const float cr = std::cos(inner), ci = -std::sin(inner);             // Complex::new(cos, sin).conj()
        const float re = x[2 * k] * cr - x[2 * k + 1] * ci;                  // num::Complex Mul
        const float im = x[2 * k] * ci + x[2 * k + 1] * cr;
        *off += change * std::atan2(im, re);                                 // pll.rs:19-21
    }
    return MODEM_OK;
}

modem_status modem_rates_sps(uint64_t br, uint64_t sr, uint64_t* sps) {   // rates.rs:12-18
    if (!sps || br == 0) return MODEM_ERR_INVALID_ARG;
    *sps = sr / br;
    return MODEM_OK;
}

float modem_carrier_phase(float w, uint64_t n) { return mod_trig(w * (float)n); }   // carrier.rs:17-19

modem_status modem_carrier_phases(float w, uint64_t s0, size_t n, float* out, int device, void* stream) {
    if (n && ptr_kind(out, device) != PTR_DEVICE) return MODEM_ERR_INVALID_ARG;
    if (!device_ok(device)) return MODEM_ERR_NO_DEVICE;
    DeviceGuard g(device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    HIP_TRY(mk::launch_phases(w, s0, n, out, (hipStream_t)stream));
    return MODEM_OK;
}

modem_status modem_phasor_bits(const modem_phasor_desc* d, uint32_t* bps) {
    if (!d || !bps) return MODEM_ERR_INVALID_ARG;
    return phasor_bps(d, bps);
}

modem_status modem_phasor_lut(const modem_phasor_desc* d, float* lut) {
    if (!d || !lut) return MODEM_ERR_INVALID_ARG;
    uint32_t bps;
    modem_status st = phasor_bps(d, &bps);
    if (st) return st;
    if (phasor_sample_dependent(d->kind)) return MODEM_ERR_UNSUPPORTED;   // no bits-only table
    if (d->kind == MODEM_PHASOR_APSK && (st = apsk_verify(d, bps))) return st;
    uint8_t b[8];
    for (uint32_t s = 0; s < (1u << bps); ++s) {
        for (uint32_t k = 0; k < bps; ++k) b[k] = (uint8_t)((s >> (bps - 1 - k)) & 1u);
        if ((st = phasor_iq(d, b, bps, &lut[2 * s], &lut[2 * s + 1]))) return st;
    }
    return MODEM_OK;
}

modem_status modem_phasor_slicer(const modem_phasor_desc* d, const float* lut, modem_slicer_desc* o) {
    if (!d || !o) return MODEM_ERR_INVALID_ARG;
    uint32_t bps;
    modem_status st = phasor_bps(d, &bps);
    if (st) return st;
    if (phasor_sample_dependent(d->kind)) return MODEM_ERR_UNSUPPORTED;
    std::memset(o, 0, sizeof *o);
    o->bits_per_symbol = bps;
    if (d->kind == MODEM_PHASOR_QAM && d->phase == 0.0f && bps % 2 == 0 && d->amplitude > 0.0f) {
        const uint32_t cs = bps / 2;
        const float ms = (float)((1u << cs) - 1);
        o->kind = MODEM_SLICER_QAM_AXIS;
        o->bits_per_carrier = cs;
        o->max_symbol = ms;
        o->inv_scale = 1.0f / (d->amplitude / ms / 2.0f);     // qam.rs:28
        return MODEM_OK;
    }
    if (!lut) return MODEM_ERR_INVALID_ARG;
    o->kind = MODEM_SLICER_NEAREST;
    o->lut = lut;
    return MODEM_OK;
}

modem_status modem_rrc_taps(uint32_t L, uint32_t sps, double beta, float* out) {
    return modem_rrc_taps_offset(L, sps, beta, 0.0, out);
}

modem_status modem_rrc_taps_offset(uint32_t L, uint32_t sps, double beta, double offset, float* out) {
    if (!out || L == 0 || sps == 0 || !(beta >= 0.0 && beta <= 1.0) || !std::isfinite(offset)) return MODEM_ERR_INVALID_ARG;
    const double pi = 3.14159265358979323846;
    std::vector<double> h(L);
    double e = 0.0;
    for (uint32_t i = 0; i < L; ++i) {
        const double t = ((double)i - (double)(L - 1) / 2.0 - offset) / (double)sps;
        double v;
        if (t == 0.0) v = 1.0 - beta + 4.0 * beta / pi;
        else if (beta > 0.0 && std::fabs(std::fabs(4.0 * beta * t) - 1.0) < 1e-12)
            v = beta / std::sqrt(2.0) * ((1.0 + 2.0 / pi) * std::sin(pi / (4.0 * beta)) +
                                         (1.0 - 2.0 / pi) * std::cos(pi / (4.0 * beta)));
        else
            v = (std::sin(pi * t * (1.0 - beta)) + 4.0 * beta * t * std::cos(pi * t * (1.0 + beta))) /
                (pi * t * (1.0 - (4.0 * beta * t) * (4.0 * beta * t)));
        h[i] = v;
        e += v * v;
    }
    const double g = 1.0 / std::sqrt(e);
    for (uint32_t i = 0; i < L; ++i) out[i] = (float)(h[i] * g);
    return MODEM_OK;
}

}  // extern "C"
